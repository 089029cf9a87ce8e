// Surface extraction by marching tetrahedra on the Kuhn split (include/invr_mesh.h states the contract), and the grid in front of the
// field query.  Five stream-ordered launches per mesh, none of which waits on another workgroup:
//   k_mesh_classify      : a 4 x 8 x 32 tile of padded points per workgroup, its inside bits (+1 halo) staged in LDS: every volume value is
//                          read once per tile -> per point the mask of crossed owned edges, per cell its triangle count (one byte each)
//   k_mesh_reduce        : per scan block of 4096 points the sums of popcount(mask) and of the triangle counts
//   k_mesh_scan_partials : ONE workgroup turns the block sums into exclusive prefixes and publishes the totals
//   k_mesh_apply         : per scan block the exclusive prefix of every point = vertex offset, triangle offset
//   k_mesh_emit          : per point its vertices (mask + offset), per cell its triangles, which find their vertex indices through
//                          offset[owner] + popcount(mask[owner] & below(slot)); every store is guarded by the caller's capacities
// A corner of a cell is named by its code q = 4 dx + 2 dy + dz; an edge slot s = 0..6 stands for the direction of code 4, 2, 1, 6, 5, 3, 7.
#include "common.h"
#include "../../include/invr_mesh.h"

#define MESH_BLOCK 256
#define MESH_TX 4
#define MESH_TY 8
#define MESH_TZ 32
#define MESH_HALO ((MESH_TX + 1) * (MESH_TY + 1) * (MESH_TZ + 1))
#define MESH_PER 16                       // points per thread of the scan kernels
static_assert(MESH_BLOCK * MESH_PER == INVR_MESH_SCAN_ITEMS, "scan block");
static_assert(MESH_TY * MESH_TZ == MESH_BLOCK, "one thread per (y, z) column of a tile");

#define MESH_CODE_OF_SLOT 0x7356124u      // nibble s = direction code of slot s
#define MESH_SLOT_OF_CODE 0x63405120u     // nibble q = slot of direction code q (q = 1..7)
// tetrahedron t = 0..5 of a cell: corners 0, A, A|B, 7 for the axis orders xyz, xzy, yxz, yzx, zxy, zyx; det[e_a, e_b, e_c] < 0 for t = 1, 2, 5
#define MESH_TET_A(t) (4u >> ((t) >> 1))
#define MESH_TET_AB(t) ((0x353656u >> (4 * (t))) & 7u)
#define MESH_TET_NEG(t) ((0x26u >> (t)) & 1u)

struct MeshDims {
    int32_t dx, dy, dz;      // the volume
    int32_t px, py, pz;      // the padded grid
    int64_t np;
};

__device__ __forceinline__ float mesh_coord(float origin, float voxel, int idx) { return origin + (float)idx * voxel; }

// value at a PADDED point: the border (and everything beyond it) and a NaN read as 0
__device__ __forceinline__ float mesh_val(const float* __restrict__ vol, const MeshDims& d, int i, int j, int k) {
    const int x = i - 1, y = j - 1, z = k - 1;
    if ((unsigned)x >= (unsigned)d.dx || (unsigned)y >= (unsigned)d.dy || (unsigned)z >= (unsigned)d.dz) return 0.0f;
    const float v = vol[((int64_t)x * d.dy + y) * d.dz + z];
    return v != v ? 0.0f : v;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_grid_points(float ox, float oy, float oz, float vx, float vy, float vz, int32_t dy, int32_t dz,
                                                           int64_t first, int64_t n, float* __restrict__ xyz) {
    const int64_t r = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (r >= n) return;
    const unsigned p = (unsigned)(first + r);          // < 2^27 (host-checked)
    const unsigned ij = p / (unsigned)dz, k = p - ij * (unsigned)dz;
    const unsigned i = ij / (unsigned)dy, j = ij - i * (unsigned)dy;
    xyz[3 * r + 0] = mesh_coord(ox, vx, (int)i);
    xyz[3 * r + 1] = mesh_coord(oy, vy, (int)j);
    xyz[3 * r + 2] = mesh_coord(oz, vz, (int)k);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_classify(const float* __restrict__ vol, MeshDims d, float level, int32_t tiles_y,
                                                             int32_t tiles_z, uint8_t* __restrict__ masks, uint8_t* __restrict__ tcounts) {
    __shared__ unsigned char s_in[MESH_HALO];
    unsigned b = blockIdx.x;
    const int tz = (int)(b % (unsigned)tiles_z);
    b /= (unsigned)tiles_z;
    const int ty = (int)(b % (unsigned)tiles_y), tx = (int)(b / (unsigned)tiles_y);
    const int i0 = tx * MESH_TX, j0 = ty * MESH_TY, k0 = tz * MESH_TZ;
    for (int e = threadIdx.x; e < MESH_HALO; e += MESH_BLOCK) {
        const int lz = e % (MESH_TZ + 1), ly = (e / (MESH_TZ + 1)) % (MESH_TY + 1), lx = e / ((MESH_TZ + 1) * (MESH_TY + 1));
        s_in[e] = mesh_val(vol, d, i0 + lx, j0 + ly, k0 + lz) >= level ? 1 : 0;
    }
    __syncthreads();
    const int lz = threadIdx.x & (MESH_TZ - 1), ly = threadIdx.x / MESH_TZ;
    const int j = j0 + ly, k = k0 + lz;
    if (j >= d.py || k >= d.pz) return;
#pragma unroll
    for (int lx = 0; lx < MESH_TX; ++lx) {
        const int i = i0 + lx;
        if (i >= d.px) break;
        unsigned c = 0;          // inside bits of the cell's corners, bit q = corner code q
#pragma unroll
        for (int q = 0; q < 8; ++q)
            c |= (unsigned)s_in[((lx + (q >> 2)) * (MESH_TY + 1) + ly + ((q >> 1) & 1)) * (MESH_TZ + 1) + lz + (q & 1)] << q;
        const unsigned in0 = c & 1u;
        unsigned mask = in0 << 7;
#pragma unroll
        for (int s = 0; s < 7; ++s) mask |= (((c >> ((MESH_CODE_OF_SLOT >> (4 * s)) & 7u)) ^ in0) & 1u) << s;
        unsigned nt = 0;
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const unsigned n = in0 + ((c >> MESH_TET_A(t)) & 1u) + ((c >> MESH_TET_AB(t)) & 1u) + (c >> 7);
            nt += (n & 1u) ? 1u : (n == 2u ? 2u : 0u);
        }
        const int64_t g = ((int64_t)i * d.py + j) * d.pz + k;
        masks[g] = (uint8_t)mask;
        tcounts[g] = (uint8_t)nt;
    }
}

// ---- the two prefix sums ----------------------------------------------------------------------------------------------------------
// 16 consecutive bytes of a per-point array as four words; bytes at and beyond np read as 0.  The arrays are allocated to a multiple of
// 16 points, so the one 16-byte load is always inside them; there is no branch on the thread's position in front of the wave scans.
__device__ __forceinline__ void mesh_load16(const uint8_t* __restrict__ arr, int64_t base, int64_t np, unsigned w[4]) {
    const int64_t last = (np + MESH_PER - 1) / MESH_PER * MESH_PER - MESH_PER;
    const uint4 v = *reinterpret_cast<const uint4*>(arr + (base < last ? base : last));
    const int valid = (int)max((int64_t)0, min(np - base, (int64_t)MESH_PER));
    const unsigned in[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = max(0, min(valid - 4 * q, 4));
        w[q] = in[q] & (k >= 4 ? 0xFFFFFFFFu : ((1u << (8 * k)) - 1u));
    }
}
__device__ __forceinline__ int mesh_vertices_of(unsigned w) { return __popc(w & 0x7F7F7F7Fu); }
__device__ __forceinline__ int mesh_triangles_of(unsigned w) { return (int)((w & 255u) + ((w >> 8) & 255u) + ((w >> 16) & 255u) + (w >> 24)); }

// exclusive prefix of x over the workgroup's MESH_BLOCK threads and the workgroup's total; every thread takes part
__device__ __forceinline__ int mesh_block_scan(int x, int* s_w, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int incl = wave_incl_sum_i(x);
    __syncthreads();                      // (s_w may still be read from the scan before)
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < MESH_BLOCK / 64; ++q) {
        before += q < wv ? s_w[q] : 0;
        all += s_w[q];
    }
    *total = all;
    return before + incl - x;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_reduce(const uint8_t* __restrict__ masks, const uint8_t* __restrict__ tcounts, int64_t np,
                                                           int32_t* __restrict__ vpart, int32_t* __restrict__ tpart) {
    __shared__ int s_w[MESH_BLOCK / 64];
    const int64_t base = ((int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x) * MESH_PER;
    unsigned m[4], c[4];
    mesh_load16(masks, base, np, m);
    mesh_load16(tcounts, base, np, c);
    int nv = 0, nt = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        nv += mesh_vertices_of(m[q]);
        nt += mesh_triangles_of(c[q]);
    }
    int vtot, ttot;
    mesh_block_scan(nv, s_w, &vtot);
    mesh_block_scan(nt, s_w, &ttot);
    if (threadIdx.x == 0) {
        vpart[blockIdx.x] = vtot;
        tpart[blockIdx.x] = ttot;
    }
}

// one workgroup: block sums -> exclusive prefixes in place, 256 at a time with a running carry; the totals to both counts arrays
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_scan_partials(int32_t* __restrict__ vpart, int32_t* __restrict__ tpart, int64_t nb,
                                                                  int64_t* __restrict__ ws_counts, int64_t* __restrict__ counts) {
    __shared__ int s_w[MESH_BLOCK / 64];
    int vcarry = 0, tcarry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += MESH_BLOCK) {
        const int64_t b = b0 + threadIdx.x, bc = b < nb ? b : nb - 1;          // (loads without a branch in front of the wave scans)
        const int vl = vpart[bc], tl = tpart[bc];
        const int v = b < nb ? vl : 0, t = b < nb ? tl : 0;
        int vtot, ttot;
        const int vex = mesh_block_scan(v, s_w, &vtot);
        const int tex = mesh_block_scan(t, s_w, &ttot);
        if (b < nb) {
            vpart[b] = vcarry + vex;
            tpart[b] = tcarry + tex;
        }
        vcarry += vtot;
        tcarry += ttot;
    }
    if (threadIdx.x < 4) {
        const int64_t v = threadIdx.x == 0 ? vcarry : threadIdx.x == 1 ? tcarry : 0;
        ws_counts[threadIdx.x] = v;
        counts[threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_apply(const uint8_t* __restrict__ masks, const uint8_t* __restrict__ tcounts, int64_t np,
                                                          const int32_t* __restrict__ vpart, const int32_t* __restrict__ tpart,
                                                          int32_t* __restrict__ voff, int32_t* __restrict__ toff) {
    __shared__ int s_w[MESH_BLOCK / 64];
    const int64_t base = ((int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x) * MESH_PER;
    unsigned m[4], c[4];
    mesh_load16(masks, base, np, m);
    mesh_load16(tcounts, base, np, c);
    int nv = 0, nt = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        nv += mesh_vertices_of(m[q]);
        nt += mesh_triangles_of(c[q]);
    }
    int tot;
    int v = vpart[blockIdx.x] + mesh_block_scan(nv, s_w, &tot);
    int t = tpart[blockIdx.x] + mesh_block_scan(nt, s_w, &tot);
    if (base >= np) return;               // (the offset arrays are allocated to a multiple of 16 points)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int4 vo, to;
        vo.x = v; to.x = t; v += __popc(m[q] & 0x7Fu); t += (int)(c[q] & 255u);
        vo.y = v; to.y = t; v += __popc(m[q] & 0x7F00u); t += (int)((c[q] >> 8) & 255u);
        vo.z = v; to.z = t; v += __popc(m[q] & 0x7F0000u); t += (int)((c[q] >> 16) & 255u);
        vo.w = v; to.w = t; v += __popc(m[q] & 0x7F000000u); t += (int)(c[q] >> 24);
        *reinterpret_cast<int4*>(voff + base + 4 * q) = vo;
        *reinterpret_cast<int4*>(toff + base + 4 * q) = to;
    }
}

// ---- emit -------------------------------------------------------------------------------------------------------------------------
struct MeshEmit {
    const float* vol;
    const uint8_t *masks, *tcounts;
    const int32_t *voff, *toff;
    const int64_t* ws_counts;
    float ox, oy, oz, vx, vy, vz, level;
    float* vertices;
    int32_t* triangles;
    int64_t vcap, tcap;
    int64_t* counts;
};

// index of the vertex on the edge between the corners of codes cp and cq (cp a subset of cq) of the cell at g
__device__ __forceinline__ int mesh_edge_vertex(const MeshEmit& a, unsigned g, unsigned sx, unsigned sy, unsigned cp, unsigned cq) {
    const unsigned o = g + ((cp >> 2) & 1u) * sx + ((cp >> 1) & 1u) * sy + (cp & 1u);
    const unsigned slot = (MESH_SLOT_OF_CODE >> (4 * (cq ^ cp))) & 7u;
    return a.voff[o] + __popc((unsigned)a.masks[o] & ((1u << slot) - 1u));
}

__device__ __forceinline__ void mesh_store_triangle(const MeshEmit& a, int64_t row, int e0, int e1, int e2, bool flip) {
    if (row >= a.tcap) return;
    a.triangles[3 * row + 0] = e0;
    a.triangles[3 * row + 1] = flip ? e2 : e1;
    a.triangles[3 * row + 2] = flip ? e1 : e2;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_emit(MeshEmit a, MeshDims d) {
    const int64_t g0 = ((int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x) * 4;
    if (g0 == 0) {
        const int64_t nv = a.ws_counts[0], nt = a.ws_counts[1];
        a.counts[0] = nv;
        a.counts[1] = nt;
        a.counts[2] = (nv > a.vcap || nt > a.tcap) ? 1 : 0;
        a.counts[3] = 0;
    }
    if (g0 >= d.np) return;
    const unsigned m4 = *reinterpret_cast<const unsigned*>(a.masks + g0), c4 = *reinterpret_cast<const unsigned*>(a.tcounts + g0);
    const unsigned sy = (unsigned)d.pz, sx = (unsigned)d.py * (unsigned)d.pz;
    for (int e = 0; e < 4; ++e) {
        const unsigned g = (unsigned)g0 + e;
        if (g >= (unsigned)d.np) break;
        const unsigned mask = (m4 >> (8 * e)) & 255u, nt = (c4 >> (8 * e)) & 255u;
        const unsigned edges = mask & 127u;
        if (edges) {
            const unsigned ij = g / (unsigned)d.pz, k = g - ij * (unsigned)d.pz;
            const unsigned i = ij / (unsigned)d.py, j = ij - i * (unsigned)d.py;
            const float va = mesh_val(a.vol, d, (int)i, (int)j, (int)k);
            const float pax = mesh_coord(a.ox, a.vx, (int)i - 1), pay = mesh_coord(a.oy, a.vy, (int)j - 1), paz = mesh_coord(a.oz, a.vz, (int)k - 1);
            int64_t row = a.voff[g];
            for (int s = 0; s < 7; ++s) {
                if (!((edges >> s) & 1u)) continue;
                const unsigned q = (MESH_CODE_OF_SLOT >> (4 * s)) & 7u;
                const int bi = (int)i + (int)(q >> 2), bj = (int)j + (int)((q >> 1) & 1u), bk = (int)k + (int)(q & 1u);
                const float vb = mesh_val(a.vol, d, bi, bj, bk);
                const float t = (a.level - va) / (vb - va);
                const float pbx = mesh_coord(a.ox, a.vx, bi - 1), pby = mesh_coord(a.oy, a.vy, bj - 1), pbz = mesh_coord(a.oz, a.vz, bk - 1);
                if (row < a.vcap) {
                    a.vertices[3 * row + 0] = pax + t * (pbx - pax);
                    a.vertices[3 * row + 1] = pay + t * (pby - pay);
                    a.vertices[3 * row + 2] = paz + t * (pbz - paz);
                }
                ++row;
            }
        }
        if (nt) {
            // the cell's corner bits from the point's own mask: corner q = inside(point) ^ crossed(edge to q)
            const unsigned in0 = mask >> 7;
            unsigned c = in0;
#pragma unroll
            for (int q = 1; q < 8; ++q) c |= (((mask >> ((MESH_SLOT_OF_CODE >> (4 * q)) & 7u)) ^ in0) & 1u) << q;
            int64_t row = a.toff[g];
            for (int t = 0; t < 6; ++t) {
                const unsigned K = (MESH_TET_A(t) << 4) | (MESH_TET_AB(t) << 8) | (7u << 12);      // nibble x = code of the path's corner x
                const unsigned bits = in0 | (((c >> MESH_TET_A(t)) & 1u) << 1) | (((c >> MESH_TET_AB(t)) & 1u) << 2) | ((c >> 7) << 3);
                const int n = __popc(bits);
                if (n == 0 || n == 4) continue;
                const bool neg = MESH_TET_NEG(t) != 0;
#define MESH_E(p, q) mesh_edge_vertex(a, g, sx, sy, (K >> (4 * (p))) & 7u, (K >> (4 * (q))) & 7u)
                if (n != 2) {
                    // one corner x against three: det[o0 - x, o1 - x, o2 - x] (others in rising order) has the sign of the tetrahedron times (-1)^x
                    const int x = __ffs((int)(n == 1 ? bits : (~bits & 15u))) - 1;
                    const int o0 = x == 0 ? 1 : 0, o1 = x <= 1 ? 2 : 1, o2 = x == 3 ? 2 : 3;
                    const int e0 = x < o0 ? MESH_E(x, o0) : MESH_E(o0, x);
                    const int e1 = x < o1 ? MESH_E(x, o1) : MESH_E(o1, x);
                    const int e2 = x < o2 ? MESH_E(x, o2) : MESH_E(o2, x);
                    mesh_store_triangle(a, row, e0, e1, e2, neg ^ ((x & 1) != 0) ^ (n == 3));
                    row += 1;
                } else {
                    // inside {p, q}, outside {r, s}: the quad pr, ps, qs, qr faces outside when (p, q, r, s) has the tetrahedron's orientation
                    const unsigned out = ~bits & 15u;
                    const int p = __ffs((int)bits) - 1, q = 31 - __clz((int)bits), r = __ffs((int)out) - 1, s = 31 - __clz((int)out);
                    const int inv = (p > r) + (p > s) + (q > r) + (q > s);
                    const bool flip = neg ^ ((inv & 1) != 0);
                    const int pr = p < r ? MESH_E(p, r) : MESH_E(r, p), ps = p < s ? MESH_E(p, s) : MESH_E(s, p);
                    const int qs = q < s ? MESH_E(q, s) : MESH_E(s, q), qr = q < r ? MESH_E(q, r) : MESH_E(r, q);
                    mesh_store_triangle(a, row, pr, ps, qs, flip);
                    mesh_store_triangle(a, row + 1, pr, qs, qr, flip);
                    row += 2;
                }
#undef MESH_E
            }
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static bool mesh_dims(const int32_t dims[3], MeshDims* d) {
    if (!dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return false;
    const int64_t px = (int64_t)dims[0] + 2, py = (int64_t)dims[1] + 2, pz = (int64_t)dims[2] + 2;
    if (px > INVR_MESH_MAX_POINTS || px * py > INVR_MESH_MAX_POINTS || px * py * pz > INVR_MESH_MAX_POINTS) return false;
    *d = MeshDims{dims[0], dims[1], dims[2], (int32_t)px, (int32_t)py, (int32_t)pz, px * py * pz};
    return true;
}

static void mesh_layout(const MeshDims& d, InvrMeshLayout* L) {
    const size_t np16 = align_up((size_t)d.np, MESH_PER);
    size_t off = 0;
    L->n_points = d.np;
    L->n_blocks = cdiv(d.np, INVR_MESH_SCAN_ITEMS);
    L->masks = (int64_t)off;    off = align_up(off + np16, 256);
    L->tcounts = (int64_t)off;  off = align_up(off + np16, 256);
    L->voffsets = (int64_t)off; off = align_up(off + np16 * sizeof(int32_t), 256);
    L->toffsets = (int64_t)off; off = align_up(off + np16 * sizeof(int32_t), 256);
    L->counts = (int64_t)off;   off = align_up(off + 4 * sizeof(int64_t), 256);
    L->partials = (int64_t)off; off = align_up(off + 2 * (size_t)L->n_blocks * sizeof(int32_t), 256);
    L->bytes = (int64_t)off;
}

extern "C" size_t invr_mesh_workspace_bytes(const int32_t dims[3]) {
    MeshDims d;
    if (!mesh_dims(dims, &d)) return 0;
    InvrMeshLayout L;
    mesh_layout(d, &L);
    return (size_t)L.bytes;
}

#define MESH_DIMS_CHECK(who)                                                                                                               \
    INVR_CHECK(dims, "%s: null dims", who);                                                                                                \
    INVR_CHECK(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1, "%s: every dimension must be >= 1 (got %d x %d x %d)", who, dims[0], dims[1], \
               dims[2]);                                                                                                                   \
    INVR_CHECK(mesh_dims(dims, &d), "%s: more than 2^27 padded points (%d x %d x %d + border)", who, dims[0], dims[1], dims[2])

extern "C" int invr_mesh_workspace_layout(const int32_t dims[3], InvrMeshLayout* layout) {
    MeshDims d;
    INVR_CHECK(layout, "invr_mesh_workspace_layout: null layout");
    MESH_DIMS_CHECK("invr_mesh_workspace_layout");
    mesh_layout(d, layout);
    return 0;
}

extern "C" int invr_grid_points(const float origin[3], const float voxel[3], const int32_t dims[3], int64_t first, int64_t n, float* xyz,
                                void* stream) {
    MeshDims d;
    INVR_CHECK(origin && voxel, "invr_grid_points: null origin / voxel");
    MESH_DIMS_CHECK("invr_grid_points");
    const int64_t total = (int64_t)dims[0] * dims[1] * dims[2];
    INVR_CHECK(first >= 0 && n >= 0 && first <= total && n <= total - first, "invr_grid_points: [first, first + n) = [%lld, %lld) leaves the grid's %lld points",
               (long long)first, (long long)(first + n), (long long)total);
    if (n == 0) return 0;
    INVR_CHECK(xyz, "invr_grid_points: null xyz");
    hipLaunchKernelGGL(k_grid_points, dim3((unsigned)cdiv(n, MESH_BLOCK)), dim3(MESH_BLOCK), 0, (hipStream_t)stream, origin[0], origin[1], origin[2],
                       voxel[0], voxel[1], voxel[2], dims[1], dims[2], first, n, xyz);
    INVR_LAUNCH_CHECK();
    return 0;
}

static int mesh_check(const char* who, const float* vol, const int32_t dims[3], float level, const void* ws, size_t ws_bytes, const int64_t* counts,
                      MeshDims* dd) {
    MeshDims d;
    MESH_DIMS_CHECK(who);
    INVR_CHECK(level > 0.0f && level <= 3.4028234e38f, "%s: level must be finite and > 0 (got %g)", who, (double)level);
    INVR_CHECK(vol && ws && counts, "%s: null volume / workspace / counts", who);
    INVR_CHECK(((uintptr_t)ws & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
    INVR_CHECK(ws_bytes >= invr_mesh_workspace_bytes(dims), "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, invr_mesh_workspace_bytes(dims));
    *dd = d;
    return 0;
}

template <class T> static T* mesh_at(void* ws, int64_t off) { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }

extern "C" int invr_mesh_count(const float* vol, const int32_t dims[3], float level, void* workspace, size_t workspace_bytes, int64_t* counts,
                               void* stream) {
    MeshDims d;
    if (mesh_check("invr_mesh_count", vol, dims, level, workspace, workspace_bytes, counts, &d)) return 1;
    InvrMeshLayout L;
    mesh_layout(d, &L);
    hipStream_t st = (hipStream_t)stream;
    uint8_t *masks = mesh_at<uint8_t>(workspace, L.masks), *tcounts = mesh_at<uint8_t>(workspace, L.tcounts);
    int32_t *vpart = mesh_at<int32_t>(workspace, L.partials), *tpart = vpart + L.n_blocks;
    const int64_t tx = cdiv(d.px, MESH_TX), ty = cdiv(d.py, MESH_TY), tz = cdiv(d.pz, MESH_TZ);
    hipLaunchKernelGGL(k_mesh_classify, dim3((unsigned)(tx * ty * tz)), dim3(MESH_BLOCK), 0, st, vol, d, level, (int32_t)ty, (int32_t)tz, masks, tcounts);
    INVR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_reduce, dim3((unsigned)L.n_blocks), dim3(MESH_BLOCK), 0, st, masks, tcounts, d.np, vpart, tpart);
    INVR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_scan_partials, dim3(1), dim3(MESH_BLOCK), 0, st, vpart, tpart, L.n_blocks, mesh_at<int64_t>(workspace, L.counts), counts);
    INVR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_apply, dim3((unsigned)L.n_blocks), dim3(MESH_BLOCK), 0, st, masks, tcounts, d.np, vpart, tpart,
                       mesh_at<int32_t>(workspace, L.voffsets), mesh_at<int32_t>(workspace, L.toffsets));
    INVR_LAUNCH_CHECK();
    return 0;
}

extern "C" int invr_mesh_emit(const float* vol, const int32_t dims[3], const float origin[3], const float voxel[3], float level, void* workspace,
                              size_t workspace_bytes, float* vertices, int64_t vertex_cap, int32_t* triangles, int64_t triangle_cap, int64_t* counts,
                              void* stream) {
    MeshDims d;
    if (mesh_check("invr_mesh_emit", vol, dims, level, workspace, workspace_bytes, counts, &d)) return 1;
    INVR_CHECK(origin && voxel, "invr_mesh_emit: null origin / voxel");
    for (int k = 0; k < 3; ++k)          // (a negative step mirrors the grid: the orientation rule is stated for a right-handed one)
        INVR_CHECK(voxel[k] > 0.0f && voxel[k] <= 3.4028234e38f, "invr_mesh_emit: voxel must be finite and > 0 in every axis (got %g)", (double)voxel[k]);
    INVR_CHECK(vertex_cap >= 0 && triangle_cap >= 0, "invr_mesh_emit: negative capacity");
    INVR_CHECK((vertex_cap == 0 || vertices) && (triangle_cap == 0 || triangles), "invr_mesh_emit: null vertices / triangles with a capacity > 0");
    InvrMeshLayout L;
    mesh_layout(d, &L);
    MeshEmit a{vol, mesh_at<uint8_t>(workspace, L.masks), mesh_at<uint8_t>(workspace, L.tcounts), mesh_at<int32_t>(workspace, L.voffsets),
               mesh_at<int32_t>(workspace, L.toffsets), mesh_at<int64_t>(workspace, L.counts), origin[0], origin[1], origin[2], voxel[0], voxel[1],
               voxel[2], level, vertices, triangles, vertex_cap, triangle_cap, counts};
    hipLaunchKernelGGL(k_mesh_emit, dim3((unsigned)cdiv(cdiv(d.np, 4), MESH_BLOCK)), dim3(MESH_BLOCK), 0, (hipStream_t)stream, a, d);
    INVR_LAUNCH_CHECK();
    return 0;
}
