/* libinvr — a surface mesh of a sampled scalar field (marching tetrahedra), entry points of libinvr.so next to include/invr.h.
 *
 * The posed occupancy field is evaluated on a regular grid (invr_grid_points feeding invr_field_fwd chunk by chunk) and the level
 * set `occupancy = level` is extracted on the device: the volume never goes to the host.
 *
 * Rules, as include/invr.h states them: plain pointers and sizes; every function returning int returns 0 on success, else a status
 * with the message in invr_last_error(); arguments are checked ahead of any launch.  All data pointers are device pointers unless
 * said otherwise; `origin`, `voxel` and `dims` are HOST arrays (as `dims` of invr_sample_volume); `stream` is a hipStream_t.  The
 * calls allocate nothing, read nothing back, launch on `stream` only and can be captured in a hipGraph.
 *
 * THE CONTRACT
 *
 * Volume and grid.  vol[Dx][Dy][Dz], fp32, x slowest, z fastest.  Grid point x(i,j,k) = origin + (i,j,k) * voxel in fp32, product
 * and sum rounded separately; voxel > 0 in every axis.
 *
 * Border.  The volume is surrounded by a virtual one-point border of value 0, never stored: the padded grid is (Dx+2, Dy+2, Dz+2),
 * padded point (i,j,k) lies at origin + (i-1, j-1, k-1) * voxel and has the padded linear index (i * (Dy+2) + j) * (Dz+2) + k.
 * `level` must be finite and > 0, so the border is outside and every surface closes.
 *
 * Inside test.  inside(v) := v >= level.  A NaN is outside and takes part in interpolation as 0 (the border's value); the other
 * values are expected to be finite.
 *
 * Cells and tetrahedra.  A cell is the cube between padded points g and g + (1,1,1) and carries g's linear index.  Its six
 * tetrahedra are the paths 000 -> +e_a -> +e_a+e_b -> 111 over the six orders (a, b, c) of the axes (the Kuhn split: translation
 * invariant, neighbouring cells agree on every shared face diagonal).
 *
 * Vertices.  One per crossed grid edge (the two ends differ in `inside`), owned by the edge's lower end g; the seven edge slots of
 * a point are g -> g + d for d in the order 100, 010, 001, 110, 101, 011, 111.  Vertex order: by the padded linear index of g,
 * then by slot.  Position p = pa + t * (pb - pa), t = (level - va) / (vb - va), a = the owning end, all fp32, computed once per
 * edge: every triangle that meets the edge uses the same index.
 *
 * Triangles.  A tetrahedron with a 1-3 split of its corners gives one triangle, a 2-2 split two, others none.  int32 indices.
 * Order: by the cell's padded linear index; inside a cell by tetrahedron in the order xyz, xzy, yxz, yzx, zxy, zyx of (a, b, c).
 * Orientation: counter-clockwise seen from outside: (p1-p0) x (p2-p0) has a non-positive dot product with the gradient of the
 * tetrahedron's linear interpolant.  The mesh is a closed, consistently oriented 2-manifold by construction.
 *
 * Determinism.  The same inputs give the same bits over any dirty workspace; there are no floating-point atomics.
 *
 * Size limit.  At most INVR_MESH_MAX_POINTS = 2^27 padded points: 7 vertices per point and 12 triangles per cell stay inside int32.
 */
#ifndef INVR_MESH_H
#define INVR_MESH_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INVR_MESH_MAX_POINTS ((int64_t)1 << 27)

/* Arrays of one extraction in the caller's workspace: BYTE offsets.  NP = (Dx+2)(Dy+2)(Dz+2) padded points in linear order. */
typedef struct InvrMeshLayout {
    int64_t masks;       /* uint8 [NP]  : bits 0..6 = crossed owned edges by slot, bit 7 = inside(point) */
    int64_t tcounts;     /* uint8 [NP]  : triangles of the cell at the point (0 where the point carries no cell) */
    int64_t voffsets;    /* int32 [NP]  : exclusive prefix sum of popcount(masks & 127): index of the point's first vertex */
    int64_t toffsets;    /* int32 [NP]  : exclusive prefix sum of tcounts: index of the cell's first triangle */
    int64_t counts;      /* int64 [4]   : {n_vertices, n_triangles, 0, 0} of the last invr_mesh_count */
    int64_t partials;    /* int32 [2][n_blocks] : exclusive prefix over the scan blocks of the vertex / triangle sums */
    int64_t n_points, n_blocks;      /* NP; scan blocks of INVR_MESH_SCAN_ITEMS points */
    int64_t bytes;
} InvrMeshLayout;

#define INVR_MESH_SCAN_ITEMS 4096

/* xyz (n, 3) = world coordinates of the points [first, first + n) of the UNPADDED grid in linear order (x slowest, z fastest):
 * the input of invr_field_fwd for one chunk of the volume. */
int invr_grid_points(const float origin[3], const float voxel[3], const int32_t dims[3], int64_t first, int64_t n, float* xyz, void* stream);

size_t invr_mesh_workspace_bytes(const int32_t dims[3]);      /* 0 for a dimension < 1 or more than INVR_MESH_MAX_POINTS padded points */
int invr_mesh_workspace_layout(const int32_t dims[3], InvrMeshLayout* layout);

/* Classify + the two prefix sums.  counts: int64 [4] on the device = {n_vertices, n_triangles, 0, 0}.  The workspace (256-byte
 * aligned) keeps what invr_mesh_emit needs. */
int invr_mesh_count(const float* vol, const int32_t dims[3], float level, void* workspace, size_t workspace_bytes, int64_t* counts, void* stream);
/* After invr_mesh_count on the same workspace, volume and level.  vertices (vertex_cap, 3) float, triangles (triangle_cap, 3) int32;
 * counts = {n_vertices, n_triangles, overflow, 0}: when a capacity is smaller than its total nothing is written past it and
 * overflow is 1. */
int invr_mesh_emit(const float* vol, const int32_t dims[3], const float origin[3], const float voxel[3], float level, void* workspace,
                   size_t workspace_bytes, float* vertices, int64_t vertex_cap, int32_t* triangles, int64_t triangle_cap, int64_t* counts,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
