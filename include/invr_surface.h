/* libinvr — the closest point on a triangle mesh for every point of a regular lattice, and barycentric interpolation of per-vertex
 * attributes there: entry points of libinvr.so next to include/invr.h.
 *
 * A subject's canonical volumes are per-vertex attributes carried to a lattice over the big-pose body by the closest point on the
 * SMPL surface (tools/prepare_zjumocap.py of the reference: get_bigpose_uv :177-240 interpolates the per-vertex UVs, get_bigpose_blend_weights
 * :312-400 the 24 skinning weights with the surface distance as channel 25).  The reference takes the closest point from
 * psbody.mesh.closest_faces_and_points (CGAL); neither is available to this project, so the result here is NOT compared with CGAL's:
 * the reference of the tests is this contract's own NumPy restatement (tests/surface_reference.py).
 *
 * Rules, as include/invr.h states them: plain pointers and sizes; every function returning int returns 0 on success, else a status
 * with the message in invr_last_error(); arguments are checked ahead of any launch.  All data pointers are device pointers unless
 * said otherwise; `origin`, `step` and `dims` are HOST arrays; `stream` is a hipStream_t.  The calls allocate nothing, read nothing
 * back, synchronise with nothing, launch on `stream` only and can be captured in a hipGraph.
 *
 * THE CONTRACT — everything in double, every operation rounded separately (no FMA).
 *
 * Lattice point.  As include/invr_posescene.h: g_a(i) = origin[a] + (double)i * step[a] for 0 <= i < dims[a].
 *
 * Dot product.  x.y = (x0*y0 + x1*y1) + x2*y2.
 *
 * Closest point on face f for the point p.  The face has the corners a, b, c = verts[faces[f][0..2]], float32 promoted to double.
 * The region walk is Ericson's (Real-Time Collision Detection, 5.1.5), in this order; the first condition that holds decides:
 *   1. ab = b - a, ac = c - a, ap = p - a; d1 = ab.ap, d2 = ac.ap.  If d1 <= 0 && d2 <= 0: (u, v, w) = (1, 0, 0).
 *   2. bp = p - b; d3 = ab.bp, d4 = ac.bp.  If d3 >= 0 && d4 <= d3: (0, 1, 0).
 *   3. vc = d1*d4 - d3*d2.  If vc <= 0 && d1 >= 0 && d3 <= 0: v = d1 / (d1 - d3), (u, v, w) = (1 - v, v, 0).
 *   4. cp = p - c; d5 = ab.cp, d6 = ac.cp.  If d6 >= 0 && d5 <= d6: (0, 0, 1).
 *   5. vb = d5*d2 - d1*d6.  If vb <= 0 && d2 >= 0 && d6 <= 0: w = d2 / (d2 - d6), (u, v, w) = (1 - w, 0, w).
 *   6. va = d3*d6 - d5*d4, e = d4 - d3, g = d5 - d6.  If va <= 0 && e >= 0 && g >= 0: w = e / (e + g), (u, v, w) = (0, 1 - w, w).
 *   7. Otherwise den = 1 / ((va + vb) + vc), v = vb * den, w = vc * den, then the clamp v = fmin(fmax(v, 0), 1),
 *      w = fmin(fmax(w, 0), 1 - v), and u = (1 - v) - w.
 * The clamp is the identity on any sane triangle; it keeps the computed point of a sliver inside its triangle up to rounding, which
 * the pruning below relies on.  fmax(x, 0) is x > 0 ? x : +0 and fmin(x, y) is x < y ? x : y here: C's functions with the NaN case
 * (a NaN v or w becomes 0) and the sign of a zero pinned.
 *
 * Point and key.  In the vertex regions 1, 2, 4 the point q is that corner exactly; otherwise q = (a + ab*v) + ac*w per component.
 * key = ((px - qx)^2 + (py - qy)^2) + (pz - qz)^2.
 *
 * Winner.  Start from (key, face) = (+inf, -1); going through the faces, face f replaces the holder when
 * key_f < key || (key_f == key && f < face): the lexicographic minimum of (key, f).  A NaN key (a zero-area face reaching a 0 / 0)
 * never wins.  A face with a corner index outside [0, n_verts) takes no part and is never dereferenced.  If no face takes part or
 * every key is NaN, the outputs are face = -1, bary = (0, 0, 0), dist = +inf.
 *
 * Outputs.  face[i] = the winner; bary[i] = its (u, v, w) as doubles; dist[i] = (float) sqrt(key): the correctly rounded double
 * square root, then round to nearest even.  Layout: [Dx][Dy][Dz], x slowest, z fastest.
 *
 * Interpolation.  For point i with f = face[i] and (u, v, w) = bary[i], channel c: A_k = attr[faces[f][k]][c] promoted to double,
 * out[i * out_stride + out_offset + c] = (float)((u*A_0 + v*A_1) + w*A_2) — barycentric_interpolation of the reference
 * (prepare_zjumocap.py:167-175: a product, sum(axis=1) over three terms, astype(float32)).  face = -1, a face outside [0, n_faces) or
 * one with a corner outside [0, n_verts) gives 0.
 *
 * Pruning.  The result is that of the brute force above over all faces, bit for bit.  The kernel prunes per tile of 4 x 4 x 4 lattice
 * points by bounding spheres of the faces against a bound taken from COMPUTED keys of a seed face, in double and widened by 2^-40
 * (csrc/k_surface.hip states the argument); there is no fp32 pre-test.
 *
 * Determinism.  No floating-point atomics, no workgroup waits on another, the same inputs give the same bits over any dirty
 * workspace and any dirty output buffers.
 *
 * Undefined input.  Vertices referenced by a face must be finite, and vertices, origin and origin + dims * step must be below 2^200
 * in magnitude (no product of two dot products overflows).  Anything else gives undefined values (but no access outside the arrays).
 *
 * Size limits.  1 <= n_verts, n_faces <= INVR_SURFACE_MAX_VERTS = INVR_SURFACE_MAX_FACES = 2^20; at most INVR_SURFACE_MAX_POINTS =
 * 2^27 points; 1 <= n_channels <= INVR_SURFACE_MAX_CHANNELS = 64; out_stride <= INVR_SURFACE_MAX_STRIDE = 2^20.
 */
#ifndef INVR_SURFACE_H
#define INVR_SURFACE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INVR_SURFACE_MAX_VERTS ((int32_t)1 << 20)
#define INVR_SURFACE_MAX_FACES ((int32_t)1 << 20)
#define INVR_SURFACE_MAX_POINTS ((int64_t)1 << 27)
#define INVR_SURFACE_MAX_CHANNELS 64
#define INVR_SURFACE_MAX_STRIDE ((int64_t)1 << 20)

/* Bytes of the workspace of one invr_surface_volume call (per face a 32-byte bounding sphere and a 48-byte corner record): 0 for
 * n_faces outside [1, 2^20]. */
size_t invr_surface_volume_workspace_bytes(int32_t n_faces);

/* verts (n_verts, 3) float32 and faces (n_faces, 3) int32 on the device; origin, step, dims on the HOST; face int32 [Dx*Dy*Dz] on the
 * device; bary float64 [Dx*Dy*Dz][3] and dist float32 [Dx*Dy*Dz] on the device, each may be NULL; the workspace 256-byte aligned and
 * of at least invr_surface_volume_workspace_bytes(n_faces). */
int invr_surface_volume(const float* verts, int32_t n_verts, const int32_t* faces, int32_t n_faces, const double origin[3],
                        const double step[3], const int32_t dims[3], int32_t* face, double* bary, float* dist, void* workspace,
                        size_t workspace_bytes, void* stream);

/* attr (n_verts, n_channels) float32, faces (n_faces, 3) int32, face int32 [n_points], bary float64 [n_points][3] and out float32 on
 * the device; writes out[i * out_stride + out_offset + c] for 0 <= i < n_points, 0 <= c < n_channels and nothing else;
 * 0 <= out_offset, out_offset + n_channels <= out_stride <= INVR_SURFACE_MAX_STRIDE.  n_points = 0 is a successful no-op. */
int invr_surface_interpolate(const float* attr, int32_t n_verts, int32_t n_channels, const int32_t* faces, int32_t n_faces,
                             const int32_t* face, const double* bary, int64_t n_points, float* out, int64_t out_stride,
                             int64_t out_offset, void* stream);

#ifdef __cplusplus
}
#endif
#endif
