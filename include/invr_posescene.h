/* libinvr — the distance volume of a posed frame, entry points of libinvr.so next to include/invr.h.
 *
 * The last channel of a frame's pose-space volume `pbw` is the distance from every point of a regular lattice over the body's box
 * to the nearest posed SMPL vertex (tools/prepare_zjumocap.py:459-499 of the reference computes it offline per frame).  The render
 * path reads no other channel of `pbw`, so a one-channel volume built here is a complete scene tensor for a new pose.
 *
 * Rules, as include/invr.h states them: plain pointers and sizes; every function returning int returns 0 on success, else a status
 * with the message in invr_last_error(); arguments are checked ahead of any launch.  All data pointers are device pointers unless
 * said otherwise; `origin`, `step` and `dims` are HOST arrays; `stream` is a hipStream_t.  The call allocates nothing, reads nothing
 * back, synchronises with nothing, launches on `stream` only and can be captured in a hipGraph.
 *
 * THE CONTRACT
 *
 * Lattice point.  g_a(i) = origin[a] + (double)i * step[a] for 0 <= i < dims[a]: one double multiply, one double add, rounded
 * separately (no FMA).  With `ax = np.arange(lo, hi + 0.025, 0.025)`, origin = ax[0] and step = ax[1] - ax[0] these are NumPy's own
 * lattice values.
 *
 * Squared distance.  For vertex row r with coordinates v (float32, promoted to double) and lattice point g:
 * d2 = ((gx - vx)^2 + (gy - vy)^2) + (gz - vz)^2 in double, every operation rounded separately, in that order.
 *
 * Winner.  The lexicographic minimum of (d2, r) over all rows: ties in d2 go to the lowest row.  nearest = that row.
 *
 * Distance.  dist = (float) sqrt(d2 of the winner): the correctly rounded double square root, then round to nearest even.
 *
 * Layout.  dist[Dx][Dy][Dz] and nearest[Dx][Dy][Dz], x slowest, z fastest: the layout of pbw[..., 0] of a (Dx, Dy, Dz, 1) volume.
 *
 * Pruning.  The result is that of the brute force above over all rows, bit for bit.  The kernel prunes per tile of 4 x 4 x 4 lattice
 * points with a bound evaluated in double and widened by 2^-40 relative (csrc/k_posescene.hip states the argument); there is no
 * fp32 pre-test.
 *
 * Determinism.  No floating-point atomics, no workgroup waits on another, the same inputs give the same bits over any dirty
 * workspace and any dirty output buffers.
 *
 * Undefined input.  Vertices must be finite, and vertices, origin and origin + dims * step must be below 2^400 in magnitude (no
 * square overflows).  Anything else gives undefined values in dist / nearest (but no access outside the arrays).
 *
 * Size limits.  1 <= n_verts <= INVR_POSESCENE_MAX_VERTS = 2^20; at most INVR_POSESCENE_MAX_POINTS = 2^27 lattice points.
 */
#ifndef INVR_POSESCENE_H
#define INVR_POSESCENE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INVR_POSESCENE_MAX_VERTS ((int32_t)1 << 20)
#define INVR_POSESCENE_MAX_POINTS ((int64_t)1 << 27)

/* Bytes of the workspace of one call (the vertices repacked as 16-byte records): 0 for n_verts outside [1, 2^20]. */
size_t invr_distance_volume_workspace_bytes(int32_t n_verts);

/* verts (n_verts, 3) float32 on the device; origin, step, dims on the HOST; dist float32 [Dx*Dy*Dz] on the device; nearest int32 of the
 * same shape on the device, or NULL; the workspace 256-byte aligned and of at least invr_distance_volume_workspace_bytes(n_verts). */
int invr_distance_volume(const float* verts, int32_t n_verts, const double origin[3], const double step[3], const int32_t dims[3],
                         float* dist, int32_t* nearest, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
