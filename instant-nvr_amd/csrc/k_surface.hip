// The closest point on a triangle mesh for every point of a regular lattice (include/invr_surface.h): the face, the barycentric
// coordinates and the distance, bit for bit the brute force of the header's contract over all faces, pruned per tile of lattice
// points; and the barycentric interpolation of per-vertex attributes at those points.
//
// k_sv_pack writes two arrays into the workspace, one entry per face: a 48-byte record {a, b, c as float32, face number} and a
// bounding sphere {s, r} in double (r < 0: the face has a corner index outside [0, V) and takes no part; its corners are never
// read).  One wave (a workgroup of 64 work-items) then owns one tile of 4 x 4 x 4 lattice points, one point per lane.  All double:
//   1. the wave finds the seed: the face whose sphere centre is nearest the tile's centre c (lowest face among equals);
//   2. every lane evaluates the contract's key of the seed for its own point; B = the maximum over the lanes, +inf if a lane's key is
//      NaN or there is no seed;
//   3. it walks the spheres and appends the records of the faces with |s - c| <= R_f = sqrt(B) + h + r_f (h = the tile's half diagonal)
//      to a candidate list in LDS (ballot compaction, so the list is in face order);
//   4. whenever another 64 might not fit, and at the end, every lane runs the contract's (key, face) minimum over the list for its
//      own point; the winner's (u, v, w) are recomputed from its record at the end (the same function on the same operands: the
//      same bits).
//
// WHY THE PRUNING IS EXACT.  Let p be a point of the tile and w the brute force's winner at p (if no key at p is a number, no face
// wins in either computation).  The brute force decides on COMPUTED keys, and Ericson's cancellations can make the computed key of a
// face much larger than its geometric distance, so no geometric distance bounds key_w.  A computed key does: key_w(p) <=
// key_seed(p) <= B whenever key_seed(p) is a number, else B = +inf.  key_w(p) is the computed |p - q|^2 for the COMPUTED point q of
// face w — a sum of three non-negative terms, each within (1 + 2^-53)^3 of its real value — so |p - q| <= sqrt(B) (1 + 2^-50), and
// with |p - c| <= h: |q - c| <= sqrt(B) + h up to 2^-50 relative.  Where is q?  Every region gives 0 <= v, w <= 1 and v + w <=
// 1 + 2^-53 (edge regions: 0 <= num <= den by the region's own conditions and monotone rounding; region 7: the clamp, with w <=
// fl(1 - v); region 6: v = fl(1 - w)), so the real point a + ab v + ac w lies in the triangle scaled by at most 1 + 2^-53 about a,
// and the computed q = (a + fl(fl(b - a) v)) + fl(fl(c - a) w) differs from it by at most 8 roundings of quantities no larger than
// 4 M, M = the largest coordinate magnitude of the face's corners: |q - real point| < 2^-46 M.  Every point of the triangle is within
// max_k |corner_k - s| of any s, so |q - s| <= r_f when the stored radius is r_f = max_k |corner_k - s| (1 + W) + W M with W = SV_WIDEN
// = 2^-40: the relative part covers the roundings of the computed radius (2^-50) and the 2^-53 scaling, the absolute part is 64
// times the error of q.  Hence |s - c| <= |s - q| + |q - c| <= r_f + sqrt(B) + h, up to 2^-50 relative in sqrt(B), h, the sum and the
// computed |s - c|^2; R_f and R_f^2 are each widened by W, a thousand times those.  So w passes the test of its tile for every p, and so
// does every face that ties with it (the argument only used key <= B).  Keys of candidates are evaluated exactly as the contract
// states them, so the (key, face) minimum over the list is the brute force's.  B = +inf tests every face that takes part (trap 2:
// a seed that reaches 0 / 0 at some lane, or no seed).  Vertices no face references enter nothing: the seed, B and the spheres are
// made of faces only.  h is taken from the computed lattice values as in k_posescene.hip; lanes outside the lattice (edge tiles)
// compute their tile's last point, so B is a maximum over points of the lattice only.
//
// Cost.  The sphere walk is 13 fp64 operations per face and lane-slot (k_posescene.hip: 8 per vertex), the key ~110 with one
// division, at the half-rate fp64 issue; the records of a list are read from LDS as broadcast 16-byte reads.  6 KB of LDS per
// wave leave room for 26 waves per CU, above what the key's registers allow (profiles/canonical_volumes.md).
#include "common.h"
#include "../../include/invr_surface.h"

#define SV_TILE 4                  // lattice points per tile and axis
#define SV_BLOCK 64                // = SV_TILE^3 = one wave: one point per lane
#define SV_CAP 128                 // candidate records in LDS (6 KB); the list is drained when fewer than 64 slots are left
#define SV_WIDEN 9.094947017729282e-13      // 2^-40
#define SV_INF __longlong_as_double(0x7FF0000000000000ll)

struct SvSphere {
    double x, y, z, r;             // r < 0: the face takes no part
};

struct SvArgs {
    const float4* rec;             // [3 n] per face {ax, ay, az, bx}, {by, bz, cx, cy}, {cz, face as int bits, 0, 0}
    const SvSphere* sph;           // [n]
    int32_t n;
    double ox, oy, oz, sx, sy, sz;
    int32_t dx, dy, dz, ty, tz;    // lattice dimensions; tiles along y and z
    int32_t* face;
    double* bary;
    float* dist;
};

__device__ __forceinline__ double sv_dot(double x0, double x1, double x2, double y0, double y1, double y2) {
    return (x0 * y0 + x1 * y1) + x2 * y2;
}

__device__ __forceinline__ double sv_d2(double gx, double gy, double gz, double vx, double vy, double vz) {
    const double ex = gx - vx, ey = gy - vy, ez = gz - vz;
    return (ex * ex + ey * ey) + ez * ez;
}

// The contract's closest point of one face for the point p -> key, and (u, v, w).  Every quantity of the region walk is evaluated
// and the first region whose condition holds selects among them (the lanes of a wave land in different regions anyway); the three
// edge quotients and region 7's reciprocal share one division, each with its own operands.
__device__ __forceinline__ double sv_closest(const float4 r0, const float4 r1, const float4 r2, double px, double py, double pz,
                                             double& u, double& v, double& w) {
    const double ax = (double)r0.x, ay = (double)r0.y, az = (double)r0.z;
    const double bx = (double)r0.w, by = (double)r1.x, bz = (double)r1.y;
    const double cx = (double)r1.z, cy = (double)r1.w, cz = (double)r2.x;
    const double abx = bx - ax, aby = by - ay, abz = bz - az;
    const double acx = cx - ax, acy = cy - ay, acz = cz - az;
    const double d1 = sv_dot(abx, aby, abz, px - ax, py - ay, pz - az), d2 = sv_dot(acx, acy, acz, px - ax, py - ay, pz - az);
    const double d3 = sv_dot(abx, aby, abz, px - bx, py - by, pz - bz), d4 = sv_dot(acx, acy, acz, px - bx, py - by, pz - bz);
    const double d5 = sv_dot(abx, aby, abz, px - cx, py - cy, pz - cz), d6 = sv_dot(acx, acy, acz, px - cx, py - cy, pz - cz);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const double e = d4 - d3, g = d5 - d6;
    const bool in1 = d1 <= 0.0 && d2 <= 0.0;
    const bool in2 = !in1 && d3 >= 0.0 && d4 <= d3;
    const bool in3 = !in1 && !in2 && vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0;
    const bool in4 = !in1 && !in2 && !in3 && d6 >= 0.0 && d5 <= d6;
    const bool in5 = !in1 && !in2 && !in3 && !in4 && vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0;
    const bool in6 = !in1 && !in2 && !in3 && !in4 && !in5 && va <= 0.0 && e >= 0.0 && g >= 0.0;
    const double num = in3 ? d1 : in5 ? d2 : in6 ? e : 1.0;
    const double den = in3 ? d1 - d3 : in5 ? d2 - d6 : in6 ? e + g : (va + vb) + vc;
    const double t = num / den;
    // region 7, clamped
    double v7 = vb * t, w7 = vc * t;
    v7 = v7 > 0.0 ? v7 : 0.0;
    v7 = v7 < 1.0 ? v7 : 1.0;
    w7 = w7 > 0.0 ? w7 : 0.0;
    const double w7max = 1.0 - v7;
    w7 = w7 < w7max ? w7 : w7max;
    v = in3 ? t : in5 ? 0.0 : in6 ? 1.0 - t : v7;
    w = in3 ? 0.0 : (in5 || in6) ? t : w7;
    u = in6 ? 0.0 : (1.0 - v) - w;          // regions 3 and 5: (1 - v) - 0 and (1 - 0) - w are the contract's 1 - v and 1 - w
    double qx = (ax + abx * v) + acx * w, qy = (ay + aby * v) + acy * w, qz = (az + abz * v) + acz * w;
    if (in1 || in2 || in4) {
        u = in1 ? 1.0 : 0.0;
        v = in2 ? 1.0 : 0.0;
        w = in4 ? 1.0 : 0.0;
        qx = in1 ? ax : in2 ? bx : cx;
        qy = in1 ? ay : in2 ? by : cy;
        qz = in1 ? az : in2 ? bz : cz;
    }
    return sv_d2(px, py, pz, qx, qy, qz);
}

__global__ void __launch_bounds__(256) k_sv_pack(const float* __restrict__ verts, int32_t n_verts, const int32_t* __restrict__ faces,
                                                 int32_t n, float4* __restrict__ rec, SvSphere* __restrict__ sph) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int i0 = faces[3 * i], i1 = faces[3 * i + 1], i2 = faces[3 * i + 2];
    float c[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    SvSphere s{0.0, 0.0, 0.0, -1.0};
    if (i0 >= 0 && i0 < n_verts && i1 >= 0 && i1 < n_verts && i2 >= 0 && i2 < n_verts) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c[k] = verts[3 * (int64_t)i0 + k];
            c[3 + k] = verts[3 * (int64_t)i1 + k];
            c[6 + k] = verts[3 * (int64_t)i2 + k];
        }
        s.x = (((double)c[0] + (double)c[3]) + (double)c[6]) * (1.0 / 3.0);
        s.y = (((double)c[1] + (double)c[4]) + (double)c[7]) * (1.0 / 3.0);
        s.z = (((double)c[2] + (double)c[5]) + (double)c[8]) * (1.0 / 3.0);
        double r2 = 0.0, m = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r2 = fmax(r2, sv_d2(s.x, s.y, s.z, (double)c[3 * k], (double)c[3 * k + 1], (double)c[3 * k + 2]));
            m = fmax(m, fmax(fabs((double)c[3 * k]), fmax(fabs((double)c[3 * k + 1]), fabs((double)c[3 * k + 2]))));
        }
        s.r = sqrt(r2) * (1.0 + SV_WIDEN) + SV_WIDEN * m;
    }
    rec[3 * (int64_t)i] = make_float4(c[0], c[1], c[2], c[3]);
    rec[3 * (int64_t)i + 1] = make_float4(c[4], c[5], c[6], c[7]);
    rec[3 * (int64_t)i + 2] = make_float4(c[8], __int_as_float(i), 0.0f, 0.0f);
    sph[i] = s;
}

// The contract's minimum over cand[0, count) for the lane's point, continuing from (best, face).
__device__ __forceinline__ void sv_drain(const float4* cand, int count, double px, double py, double pz, double& best, int& face) {
    for (int k = 0; k < count; ++k) {
        const float4 r2 = cand[3 * k + 2];
        double u, v, w;
        const double key = sv_closest(cand[3 * k], cand[3 * k + 1], r2, px, py, pz, u, v, w);
        const int f = __float_as_int(r2.y);
        if (key < best || (key == best && f < face)) {
            best = key;
            face = f;
        }
    }
}

__global__ void __launch_bounds__(SV_BLOCK) k_sv_tiles(SvArgs a) {
    __shared__ float4 cand[3 * SV_CAP];
    const int lane = threadIdx.x;
    int t = blockIdx.x;
    const int tz = t % a.tz; t /= a.tz;
    const int ty = t % a.ty; t /= a.ty;
    const int x0 = t * SV_TILE, y0 = ty * SV_TILE, z0 = tz * SV_TILE;
    const int x1 = min(x0 + SV_TILE - 1, a.dx - 1), y1 = min(y0 + SV_TILE - 1, a.dy - 1), z1 = min(z0 + SV_TILE - 1, a.dz - 1);
    // the lane's point; a lane outside the lattice (edge tiles) computes its tile's last point along that axis and stores nothing
    const int ix = x0 + (lane >> 4), iy = y0 + ((lane >> 2) & 3), iz = z0 + (lane & 3);
    const bool inside = ix < a.dx && iy < a.dy && iz < a.dz;
    const double px = a.ox + (double)min(ix, x1) * a.sx, py = a.oy + (double)min(iy, y1) * a.sy, pz = a.oz + (double)min(iz, z1) * a.sz;
    // tile centre and half extents from the computed end points
    const double ax = a.ox + (double)x0 * a.sx, bx = a.ox + (double)x1 * a.sx;
    const double ay = a.oy + (double)y0 * a.sy, by = a.oy + (double)y1 * a.sy;
    const double az = a.oz + (double)z0 * a.sz, bz = a.oz + (double)z1 * a.sz;
    const double cx = 0.5 * (ax + bx), cy = 0.5 * (ay + by), cz = 0.5 * (az + bz);
    const double hx = fmax(bx - cx, cx - ax), hy = fmax(by - cy, cy - ay), hz = fmax(bz - cz, cz - az);
    const double h = sqrt((hx * hx + hy * hy) + hz * hz);

    // 1. the seed: the lexicographic minimum of (|s - c|^2, face) over the faces that take part
    double m2 = SV_INF;
    int seed = -1;
    for (int i = lane; i < a.n; i += SV_BLOCK) {
        const SvSphere s = a.sph[i];
        const double d2 = sv_d2(cx, cy, cz, s.x, s.y, s.z);
        if (s.r >= 0.0 && d2 < m2) {          // (ascending i: the lane keeps the lowest face among equals)
            m2 = d2;
            seed = i;
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const double om = __shfl_xor(m2, s);
        const int os = __shfl_xor(seed, s);
        if (os >= 0 && (seed < 0 || om < m2 || (om == m2 && os < seed))) {
            m2 = om;
            seed = os;
        }
    }
    // 2. B from the seed's computed keys
    double B = SV_INF;
    if (seed >= 0) {
        double u, v, w;
        B = sv_closest(a.rec[3 * (int64_t)seed], a.rec[3 * (int64_t)seed + 1], a.rec[3 * (int64_t)seed + 2], px, py, pz, u, v, w);
        B = B == B ? B : SV_INF;
    }
    for (int s = 32; s >= 1; s >>= 1) B = fmax(B, __shfl_xor(B, s));
    const double reach = sqrt(B) + h;

    // 3. + 4. candidates in face order, drained whenever another 64 might not fit
    double best = SV_INF;
    int face = -1;
    int count = 0;
    for (int base = 0; base < a.n; base += SV_BLOCK) {
        const int i = base + lane;
        bool pass = false;
        if (i < a.n) {
            const SvSphere s = a.sph[i];
            const double R = (reach + s.r) * (1.0 + SV_WIDEN);
            pass = s.r >= 0.0 && sv_d2(cx, cy, cz, s.x, s.y, s.z) <= (R * R) * (1.0 + SV_WIDEN);
        }
        const unsigned long long mask = __ballot(pass);
        if (pass) {
            const int k = count + __popcll(mask & ((1ull << lane) - 1ull));
            cand[3 * k] = a.rec[3 * (int64_t)i];
            cand[3 * k + 1] = a.rec[3 * (int64_t)i + 1];
            cand[3 * k + 2] = a.rec[3 * (int64_t)i + 2];
        }
        count += __popcll(mask);
        if (count + SV_BLOCK > SV_CAP) {
            __syncthreads();
            sv_drain(cand, count, px, py, pz, best, face);
            __syncthreads();
            count = 0;
        }
    }
    __syncthreads();
    sv_drain(cand, count, px, py, pz, best, face);

    if (inside) {
        const int64_t o = ((int64_t)ix * a.dy + iy) * a.dz + iz;
        a.face[o] = face;
        if (a.dist) a.dist[o] = (float)sqrt(best);
        if (a.bary) {
            double u = 0.0, v = 0.0, w = 0.0;
            if (face >= 0) sv_closest(a.rec[3 * (int64_t)face], a.rec[3 * (int64_t)face + 1], a.rec[3 * (int64_t)face + 2], px, py, pz, u, v, w);
            a.bary[3 * o] = u;
            a.bary[3 * o + 1] = v;
            a.bary[3 * o + 2] = w;
        }
    }
}

// One work-item per (point, channel).
__global__ void __launch_bounds__(256) k_sv_interpolate(const float* __restrict__ attr, int32_t n_verts, int32_t nc,
                                                        const int32_t* __restrict__ faces, int32_t n_faces, const int32_t* __restrict__ face,
                                                        const double* __restrict__ bary, int64_t total, float* __restrict__ out,
                                                        int64_t out_stride, int64_t out_offset) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    const int64_t i = j / nc;
    const int c = (int)(j - i * nc);
    const int f = face[i];
    float r = 0.0f;
    if (f >= 0 && f < n_faces) {
        const int i0 = faces[3 * (int64_t)f], i1 = faces[3 * (int64_t)f + 1], i2 = faces[3 * (int64_t)f + 2];
        if (i0 >= 0 && i0 < n_verts && i1 >= 0 && i1 < n_verts && i2 >= 0 && i2 < n_verts) {
            const double u = bary[3 * i], v = bary[3 * i + 1], w = bary[3 * i + 2];
            const double a0 = (double)attr[(int64_t)i0 * nc + c], a1 = (double)attr[(int64_t)i1 * nc + c], a2 = (double)attr[(int64_t)i2 * nc + c];
            r = (float)((u * a0 + v * a1) + w * a2);
        }
    }
    out[i * out_stride + out_offset + c] = r;
}

static size_t sv_rec_bytes(int32_t n_faces) { return align_up((size_t)n_faces * 3 * sizeof(float4), 256); }

extern "C" size_t invr_surface_volume_workspace_bytes(int32_t n_faces) {
    if (n_faces < 1 || n_faces > INVR_SURFACE_MAX_FACES) return 0;
    return sv_rec_bytes(n_faces) + align_up((size_t)n_faces * sizeof(SvSphere), 256);
}

extern "C" int invr_surface_volume(const float* verts, int32_t n_verts, const int32_t* faces, int32_t n_faces, const double origin[3],
                                   const double step[3], const int32_t dims[3], int32_t* face, double* bary, float* dist, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    const char* who = "invr_surface_volume";
    INVR_CHECK(verts && faces && origin && step && dims && face && workspace, "%s: null verts / faces / origin / step / dims / face / workspace", who);
    INVR_CHECK(n_verts >= 1 && n_verts <= INVR_SURFACE_MAX_VERTS, "%s: n_verts must be in [1, 2^20] (got %d)", who, n_verts);
    INVR_CHECK(n_faces >= 1 && n_faces <= INVR_SURFACE_MAX_FACES, "%s: n_faces must be in [1, 2^20] (got %d)", who, n_faces);
    INVR_CHECK(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1, "%s: every dimension must be >= 1 (got %d x %d x %d)", who, dims[0], dims[1], dims[2]);
    INVR_CHECK((int64_t)dims[0] * dims[1] <= INVR_SURFACE_MAX_POINTS && (int64_t)dims[0] * dims[1] * dims[2] <= INVR_SURFACE_MAX_POINTS,
               "%s: more than 2^27 lattice points (%d x %d x %d)", who, dims[0], dims[1], dims[2]);
    for (int k = 0; k < 3; ++k) {
        INVR_CHECK(step[k] > 0.0 && step[k] <= 1.7976931348623157e308, "%s: step must be finite and > 0 in every axis (got %g)", who, step[k]);
        INVR_CHECK(origin[k] >= -1.7976931348623157e308 && origin[k] <= 1.7976931348623157e308, "%s: origin must be finite (got %g)", who, origin[k]);
    }
    INVR_CHECK(((uintptr_t)workspace & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
    const size_t need = invr_surface_volume_workspace_bytes(n_faces);
    INVR_CHECK(workspace_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    float4* rec = static_cast<float4*>(workspace);
    SvSphere* sph = reinterpret_cast<SvSphere*>(static_cast<char*>(workspace) + sv_rec_bytes(n_faces));
    hipLaunchKernelGGL(k_sv_pack, dim3((unsigned)cdiv(n_faces, 256)), dim3(256), 0, st, verts, n_verts, faces, n_faces, rec, sph);
    INVR_LAUNCH_CHECK();
    const int64_t tx = cdiv(dims[0], SV_TILE), ty = cdiv(dims[1], SV_TILE), tz = cdiv(dims[2], SV_TILE);
    SvArgs a{rec, sph, n_faces, origin[0], origin[1], origin[2], step[0], step[1], step[2], dims[0], dims[1], dims[2], (int32_t)ty, (int32_t)tz,
             face, bary, dist};
    hipLaunchKernelGGL(k_sv_tiles, dim3((unsigned)(tx * ty * tz)), dim3(SV_BLOCK), 0, st, a);
    INVR_LAUNCH_CHECK();
    return 0;
}

extern "C" int invr_surface_interpolate(const float* attr, int32_t n_verts, int32_t n_channels, const int32_t* faces, int32_t n_faces,
                                        const int32_t* face, const double* bary, int64_t n_points, float* out, int64_t out_stride,
                                        int64_t out_offset, void* stream) {
    const char* who = "invr_surface_interpolate";
    INVR_CHECK(n_verts >= 1 && n_verts <= INVR_SURFACE_MAX_VERTS, "%s: n_verts must be in [1, 2^20] (got %d)", who, n_verts);
    INVR_CHECK(n_faces >= 1 && n_faces <= INVR_SURFACE_MAX_FACES, "%s: n_faces must be in [1, 2^20] (got %d)", who, n_faces);
    INVR_CHECK(n_channels >= 1 && n_channels <= INVR_SURFACE_MAX_CHANNELS, "%s: n_channels must be in [1, 64] (got %d)", who, n_channels);
    INVR_CHECK(n_points >= 0 && n_points <= INVR_SURFACE_MAX_POINTS, "%s: n_points must be in [0, 2^27] (got %lld)", who, (long long)n_points);
    INVR_CHECK(out_offset >= 0 && out_stride >= n_channels && out_stride <= INVR_SURFACE_MAX_STRIDE && out_offset <= out_stride - n_channels,
               "%s: need 0 <= out_offset, out_offset + n_channels <= out_stride <= 2^20 (got offset %lld, stride %lld, %d channels)", who,
               (long long)out_offset, (long long)out_stride, n_channels);
    if (n_points == 0) return 0;
    INVR_CHECK(attr && faces && face && bary && out, "%s: null attr / faces / face / bary / out", who);
    const int64_t total = n_points * n_channels;
    hipLaunchKernelGGL(k_sv_interpolate, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, attr, n_verts, n_channels, faces,
                       n_faces, face, bary, total, out, out_stride, out_offset);
    INVR_LAUNCH_CHECK();
    return 0;
}
