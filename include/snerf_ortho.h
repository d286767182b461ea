/*
 * snerf_ortho.h -- geo-referenced ortho products on the DSM lattice: the top-surface z-buffer of a UTM (east, north, alt) cloud
 * with the colour, label or any scalar of the winning point, and per-cell label votes.  Compiled into libsnerf_hip.so beside the
 * entries of snerf_hip.h, whose conventions hold here (device pointers, 0 = success, snerf_last_error() gives the message, no
 * allocation and no synchronisation, asynchronous on `stream`).  The reference has no counterpart; the spec is this header
 * and DESIGN.md section 5j, and tests/ortho_numpy.py restates it in numpy integer arithmetic.
 *
 * Lattice: exactly snerf_dsm_accumulate's (SnerfDsmGrid).  A point (x, y, z) has the cell i = floor((x - xoff)/res),
 * j = floor((yoff - y)/res) in fp64 and OFFERS itself to every cell (i+kx, j+ky), |kx|, |ky| <= radius, that lies inside the
 * lattice extent [0, xsize) x [0, ysize) AND inside the output window (ioff, joff, out_w, out_h) -- also when its own cell lies
 * outside.  A point whose x or y is not finite offers nothing.  radius lies in [0, 7].  cells = out_h * out_w, row-major, row 0
 * at the north edge.
 *
 * Everything is integer arithmetic on the device (integer atomic max / add only, no float atomics), so every result is
 * bit-reproducible and independent of launch order, of how a cloud is cut into calls, of the order of the calls and of ranks.
 *
 * Refused by every entry without touching the device: null required pointers, n outside [0, 2^31], radius outside [0, 7],
 * n_classes outside [1, 255], a grid without res > 0 and positive sizes, a window that reaches beyond int32 cell indices, q not
 * positive and finite, z0 not finite, index0 < 0 or index0 + n > 2^32 - 1, cells < 1, a payload pair given by halves.
 * n = 0 is legal and launches nothing.
 */
#ifndef SNERF_ORTHO_H
#define SNERF_ORTHO_H

#include "snerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_ORTHO_VERSION 1
#define SNERF_ORTHO_MAX_RADIUS 7
#define SNERF_ORTHO_MAX_CLASSES 255
#define SNERF_ORTHO_NO_LABEL 255   /* label_out of a cell without a winner / vote, and of a label outside [0, 254] */

int snerf_ortho_version(void);

/* Top-surface z-buffer.  xyz (n, 3) fp64; top[cells] (u64, ZEROED by the caller before the first call, accumulated).
 * Per point p: k = llrint((z - z0)/q) (ties to even), which must lie in [-2^31, 2^31); the key
 *   ((u64)(k + 2^31) << 32) | (0xFFFFFFFF - (index0 + p))
 * enters every offered cell by an integer atomic max: the highest quantised altitude wins and, on a tie, the LOWEST global
 * point index.  0 = no point (no valid key is 0: index0 + n <= 2^32 - 1).  Keys commute; ranks combine by a MAX all-reduce.
 * stats[4] (u64, zeroed by the caller, accumulated): [0] += points whose quantised altitude is not finite or out of range (they
 * offer nothing, whatever their x, y); [1] += points that reached at least one cell; [2], [3] reserved. */
int snerf_ortho_top(const double* xyz, long long n, long long index0, const SnerfDsmGrid* grid, int radius, double z0, double q,
                    unsigned long long* top, unsigned long long* stats, void* stream);

/* One thread per cell.  alt_out[c] = f32(z0 + q*k) (NaN when top[c] = 0) and idx_out[c] = the winner's global index (int64, -1
 * when empty) are written for every cell.  The payload outputs are written ONLY where the winner's index lies in
 * [index0, index0 + n), from row (index - index0) of the payload inputs: a fused map gathers once per image into buffers the
 * caller pre-filled.  rgb (n, 3) fp32 -> rgb_out (3, cells) fp32; labels (n) int64 -> label_out (cells) u8, a label outside
 * [0, 254] written as 255; scalar (n) fp32 -> scalar_out (cells) fp32.  Each payload pair may be NULL (both pointers). */
int snerf_ortho_gather(const unsigned long long* top, long long cells, long long index0, long long n, double z0, double q,
                       const float* rgb, const long long* labels, const float* scalar, float* alt_out, long long* idx_out,
                       float* rgb_out, unsigned char* label_out, float* scalar_out, void* stream);

/* Label votes: votes[label * cells + cell] (u32, zeroed by the caller, accumulated) += 1 for every offered cell of every point
 * whose label (int64) lies in [0, n_classes) and whose x, y are finite; z is not read.  stats[4] (u64, zeroed by the caller):
 * [0] += points with a label outside [0, n_classes) or a non-finite x or y (they vote nowhere). */
int snerf_ortho_votes(const double* xyz, const long long* labels, long long n, const SnerfDsmGrid* grid, int radius, int n_classes,
                      unsigned* votes, unsigned long long* stats, void* stream);

/* One thread per cell: label_out[c] (u8) = the class with the most votes, the LOWEST class on a tie, 255 when the cell has no
 * vote; share_out[c] = f32((double)max / (double)total), NaN when empty; stats[1] = max(stats[1], the largest total of a cell).
 * A class count cannot have wrapped iff stats[1] < 2^32: the caller checks this on the host. */
int snerf_ortho_votes_finish(const unsigned* votes, int n_classes, long long cells, unsigned char* label_out, float* share_out,
                             unsigned long long* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SNERF_ORTHO_H */
