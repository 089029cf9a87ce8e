// The distance volume of a posed frame (include/invr_posescene.h): for every point of a regular lattice the distance to the nearest
// vertex and that vertex's row, bit for bit the brute force of the header's contract, pruned per tile of lattice points.
//
// One wave (a workgroup of 64 work-items) owns one tile of 4 x 4 x 4 lattice points, one point per lane.  Everything is double:
//   1. the wave finds m2 = min over all vertices of the squared distance to the tile's centre c;
//   2. it walks the vertices again and appends those with |v - c|^2 <= R2 to a candidate list in LDS (ballot compaction, so the list is
//      in row order), R = sqrt(m2) + 2 h, h = the tile's half diagonal;
//   3. whenever the list is full, and at the end, every lane runs the contract's (d2, row) minimum over the list for its own point.
// The vertices are read as 16-byte records {x, y, z, row} which k_dv_pack writes into the workspace ahead of the tile kernel.
//
// WHY THE PRUNING IS EXACT.  Let p be a point of the tile, u the vertex nearest to c, w the brute force's winner at p.  In real
// arithmetic |p - c| <= h, so |w - p| <= |u - p| <= |u - c| + h and |w - c| <= |w - p| + h <= |u - c| + 2 h = R.  The computed
// quantities differ from the real ones by rounding: a computed squared distance is a sum of three non-negative terms, each within
// (1 + 2^-53)^3 of its real value, so it is within 2^-50 relative of the real one, and so are sqrt(m2), h, R and R2 after a handful
// more operations.  The brute force's winner is decided on computed keys, which moves |w - p| <= |u - p| by the same 2^-50.  R and R2
// are therefore each widened by DV_WIDEN = 2^-40 relative, a thousand times every rounding error in the chain; a vertex that fails
// the widened test cannot hold the minimal key at any point of the tile, and u itself always passes (R2 >= m2), so the list is never
// empty.  Keys of candidates are evaluated exactly as the contract states them, so ties and their rows are the brute force's.
// h is taken from the computed lattice values themselves (monotone in the index because rounding is monotone and step > 0): per axis
// the larger of the two computed differences between c and the tile's end points.
#include "common.h"
#include "../../include/invr_posescene.h"

#define DV_TILE 4                  // lattice points per tile and axis
#define DV_BLOCK 64                // = DV_TILE^3 = one wave: one point per lane
#define DV_CAP 256                 // candidate records in LDS (4 KB: 8 waves per SIMD); the list is drained when fewer than 64 slots are left
#define DV_WIDEN 9.094947017729282e-13      // 2^-40

struct DvArgs {
    const float4* rec;             // [n] {x, y, z, row as int bits}
    int32_t n;
    double ox, oy, oz, sx, sy, sz;
    int32_t dx, dy, dz, ty, tz;    // lattice dimensions; tiles along y and z
    float* dist;
    int32_t* nearest;
};

__global__ void __launch_bounds__(256) k_dv_pack(const float* __restrict__ verts, int32_t n, float4* __restrict__ rec) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) rec[i] = make_float4(verts[3 * i], verts[3 * i + 1], verts[3 * i + 2], __int_as_float(i));
}

__device__ __forceinline__ double dv_d2(double gx, double gy, double gz, double vx, double vy, double vz) {
    const double ex = gx - vx, ey = gy - vy, ez = gz - vz;
    return (ex * ex + ey * ey) + ez * ez;
}

// The contract's minimum over cand[0, count) for the lane's point, continuing from (best, row).
__device__ __forceinline__ void dv_drain(const float4* cand, int count, double gx, double gy, double gz, double& best, int& row) {
    for (int k = 0; k < count; ++k) {
        const float4 v = cand[k];
        const double d2 = dv_d2(gx, gy, gz, (double)v.x, (double)v.y, (double)v.z);
        const int r = __float_as_int(v.w);
        if (d2 < best || (d2 == best && r < row)) {
            best = d2;
            row = r;
        }
    }
}

__global__ void __launch_bounds__(DV_BLOCK) k_dv_tiles(DvArgs a) {
    __shared__ float4 cand[DV_CAP];
    const int lane = threadIdx.x;
    int t = blockIdx.x;
    const int tz = t % a.tz; t /= a.tz;
    const int ty = t % a.ty; t /= a.ty;
    const int x0 = t * DV_TILE, y0 = ty * DV_TILE, z0 = tz * DV_TILE;
    const int x1 = min(x0 + DV_TILE - 1, a.dx - 1), y1 = min(y0 + DV_TILE - 1, a.dy - 1), z1 = min(z0 + DV_TILE - 1, a.dz - 1);
    // the lane's point; a lane outside the lattice (edge tiles) computes its tile's last point along that axis and stores nothing
    const int ix = x0 + (lane >> 4), iy = y0 + ((lane >> 2) & 3), iz = z0 + (lane & 3);
    const bool inside = ix < a.dx && iy < a.dy && iz < a.dz;
    const double gx = a.ox + (double)min(ix, x1) * a.sx, gy = a.oy + (double)min(iy, y1) * a.sy, gz = a.oz + (double)min(iz, z1) * a.sz;
    // tile centre and half extents from the computed end points
    const double ax = a.ox + (double)x0 * a.sx, bx = a.ox + (double)x1 * a.sx;
    const double ay = a.oy + (double)y0 * a.sy, by = a.oy + (double)y1 * a.sy;
    const double az = a.oz + (double)z0 * a.sz, bz = a.oz + (double)z1 * a.sz;
    const double cx = 0.5 * (ax + bx), cy = 0.5 * (ay + by), cz = 0.5 * (az + bz);
    const double hx = fmax(bx - cx, cx - ax), hy = fmax(by - cy, cy - ay), hz = fmax(bz - cz, cz - az);
    const double h = sqrt((hx * hx + hy * hy) + hz * hz);

    // 1. squared distance from the centre to its nearest vertex
    double m2 = __longlong_as_double(0x7FF0000000000000ll);
    for (int i = lane; i < a.n; i += DV_BLOCK) {
        const float4 v = a.rec[i];
        m2 = fmin(m2, dv_d2(cx, cy, cz, (double)v.x, (double)v.y, (double)v.z));
    }
    for (int s = 32; s >= 1; s >>= 1) m2 = fmin(m2, __shfl_xor(m2, s));
    const double R = (sqrt(m2) + 2.0 * h) * (1.0 + DV_WIDEN);
    const double R2 = (R * R) * (1.0 + DV_WIDEN);

    // 2. + 3. candidates in row order, drained whenever another 64 might not fit
    double best = __longlong_as_double(0x7FF0000000000000ll);
    int row = 0;
    int count = 0;
    for (int base = 0; base < a.n; base += DV_BLOCK) {
        const int i = base + lane;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        bool pass = false;
        if (i < a.n) {
            v = a.rec[i];
            pass = dv_d2(cx, cy, cz, (double)v.x, (double)v.y, (double)v.z) <= R2;
        }
        const unsigned long long mask = __ballot(pass);
        if (pass) cand[count + __popcll(mask & ((1ull << lane) - 1ull))] = v;
        count += __popcll(mask);
        if (count + DV_BLOCK > DV_CAP) {
            __syncthreads();
            dv_drain(cand, count, gx, gy, gz, best, row);
            __syncthreads();
            count = 0;
        }
    }
    __syncthreads();
    dv_drain(cand, count, gx, gy, gz, best, row);

    if (inside) {
        const int64_t o = ((int64_t)ix * a.dy + iy) * a.dz + iz;
        a.dist[o] = (float)sqrt(best);
        if (a.nearest) a.nearest[o] = row;
    }
}

extern "C" size_t invr_distance_volume_workspace_bytes(int32_t n_verts) {
    if (n_verts < 1 || n_verts > INVR_POSESCENE_MAX_VERTS) return 0;
    return align_up((size_t)n_verts * sizeof(float4), 256);
}

extern "C" int invr_distance_volume(const float* verts, int32_t n_verts, const double origin[3], const double step[3], const int32_t dims[3],
                                    float* dist, int32_t* nearest, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "invr_distance_volume";
    INVR_CHECK(verts && origin && step && dims && dist && workspace, "%s: null verts / origin / step / dims / dist / workspace", who);
    INVR_CHECK(n_verts >= 1 && n_verts <= INVR_POSESCENE_MAX_VERTS, "%s: n_verts must be in [1, 2^20] (got %d)", who, n_verts);
    INVR_CHECK(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1, "%s: every dimension must be >= 1 (got %d x %d x %d)", who, dims[0], dims[1], dims[2]);
    INVR_CHECK((int64_t)dims[0] * dims[1] <= INVR_POSESCENE_MAX_POINTS && (int64_t)dims[0] * dims[1] * dims[2] <= INVR_POSESCENE_MAX_POINTS,
               "%s: more than 2^27 lattice points (%d x %d x %d)", who, dims[0], dims[1], dims[2]);
    for (int k = 0; k < 3; ++k) {
        INVR_CHECK(step[k] > 0.0 && step[k] <= 1.7976931348623157e308, "%s: step must be finite and > 0 in every axis (got %g)", who, step[k]);
        INVR_CHECK(origin[k] >= -1.7976931348623157e308 && origin[k] <= 1.7976931348623157e308, "%s: origin must be finite (got %g)", who, origin[k]);
    }
    INVR_CHECK(((uintptr_t)workspace & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
    const size_t need = invr_distance_volume_workspace_bytes(n_verts);
    INVR_CHECK(workspace_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    float4* rec = static_cast<float4*>(workspace);
    hipLaunchKernelGGL(k_dv_pack, dim3((unsigned)cdiv(n_verts, 256)), dim3(256), 0, st, verts, n_verts, rec);
    INVR_LAUNCH_CHECK();
    const int64_t tx = cdiv(dims[0], DV_TILE), ty = cdiv(dims[1], DV_TILE), tz = cdiv(dims[2], DV_TILE);
    DvArgs a{rec, n_verts, origin[0], origin[1], origin[2], step[0], step[1], step[2], dims[0], dims[1], dims[2], (int32_t)ty, (int32_t)tz, dist, nearest};
    hipLaunchKernelGGL(k_dv_tiles, dim3((unsigned)(tx * ty * tz)), dim3(DV_BLOCK), 0, st, a);
    INVR_LAUNCH_CHECK();
    return 0;
}
