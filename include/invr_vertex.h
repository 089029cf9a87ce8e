/* libinvr — de-hashed vertex tables of the eval encoder, entry points of libinvr.so next to include/invr.h.
 *
 * For a grid with row sums (invr_grid_row_sums) the value of a hashed level at its grid vertex (cx, cy, cz) is
 * row_sums[level l's first row + hash(cx, cy, cz) mod T]: a constant of the model, like the row sums themselves.  For every hashed
 * level l (in level order) with res_l^3 <= max_rows these calls lay out a dense table
 *     V_l[(cx res_l + cy) res_l + cz] = row_sums[first row of l + hash(cx, cy, cz) mod T]
 * back to back, two zero floats behind the last.  A level read through its table is an ordinary dense level of the row-sum encoder
 * kernels (no hash arithmetic, neighbouring vertices in neighbouring floats) and gives the same bits.
 *
 * max_rows in [0, INVR_VERTEX_MAX_ROWS]: 2^24 vertices give res <= 256, which keeps the 24-bit multiplies of the dense route in range;
 * more is refused.  invr_grid_vertex_sums_len = number of floats (0: no level qualifies, -1: max_rows above the limit).
 * invr_grid_vertex_sums fills `out` (DEVICE, that many floats) from grid->row_sums on `stream`; grid->vertex_rows is not read.
 *
 * To have the encoder read them (InvrGrid.vertex_rows): allocate invr_grid_row_sums_len + invr_grid_vertex_sums_len floats, fill the
 * front with invr_grid_row_sums, point grid->row_sums at it, build the tables into the floats behind it and set grid->vertex_rows =
 * max_rows.  Rebuild them whenever the row sums are rebuilt.
 *
 * Rules, as include/invr.h states them: 0 on success, else a status with the message in invr_last_error(). */
#ifndef INVR_VERTEX_H
#define INVR_VERTEX_H

#include "invr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INVR_VERTEX_MAX_ROWS 16777216

int64_t invr_grid_vertex_sums_len(const InvrGrid* grid, int64_t max_rows);
int invr_grid_vertex_sums(const InvrGrid* grid, int64_t max_rows, float* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
