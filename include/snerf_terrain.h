/* Extension of the C-ABI of libsnerf_hip.so: bare-earth terrain on the map -- a progressive morphological ground filter (Zhang et
 * al. 2003) on the integer altitude keys of a raster, and a scan-line fill of the ground under everything that is not ground: the
 * DTM, the height above ground nDSM = DSM - DTM and the ground mask.  A map product of this project (the reference has no
 * counterpart); DESIGN.md section 5y, restated in numpy by tests/terrain_numpy.py.
 *
 * include/snerf_hip.h is the ABI-6 surface and its list of entry points is frozen; an entry added at the same ABI version is
 * declared in a header of its own (as include/snerf_objects.h), which includes it for the error codes and the limits.  Same
 * conventions: plain pointers + sizes, device pointers unless stated, `stream` is a hipStream_t, 0 = SNERF_OK, a message for every
 * other return through snerf_last_error(); no entry allocates or synchronises with the host, and none launches anything for an
 * empty problem.  snerf_version() stays 6.
 * The Python binding is this header's group of rows in _lib.HEADER_SIGNATURES (tests/test_terrain_cpu.py compares it with this file).
 *
 * A raster is (h, w), row 0 the north edge, cell c = j * w + i (row j, column i); h * w < 2^31.
 * An altitude becomes a key k = rint((alt - z0) / q) in fp64, as the lattice's keys quantise.  A key is valid in the OPEN range
 * (-2^31, 2^31 - 1); the stored hole is SNERF_TERRAIN_HOLE (2^31 - 1 is no key either, and is read as a hole).
 * A class table is a HOST array of 256 bytes, entry c non-zero = class c is in the set; it goes to the kernel by value.  Class 255
 * (SNERF_ORTHO_NO_LABEL) is in no set: a table that names it is refused.
 * `flags` is one byte per cell:  bit 0 (SNERF_TERRAIN_FLAGGED) flagged by the filter,  bit 1 (SNERF_TERRAIN_BLOCKED) blocked by
 * its class,  bit 2 (SNERF_TERRAIN_IS_HOLE) a hole.  A cell is ground if and only if its flags are 0.
 * Every kernel's loops are counted by h, w and radius alone; nothing terminates on memory content; the only atomics are the integer
 * counts of `stats`, which the caller zeroes and the entries only add to. */
#ifndef SNERF_TERRAIN_H
#define SNERF_TERRAIN_H

#include "snerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_TERRAIN_HOLE (-2147483647 - 1)
#define SNERF_TERRAIN_MAX_RADIUS 512
#define SNERF_TERRAIN_FLAGGED 1
#define SNERF_TERRAIN_BLOCKED 2
#define SNERF_TERRAIN_IS_HOLE 4

/* snerf_terrain_workspace_bytes: HOST only.  The bytes of `ws` that snerf_terrain_open (two int32 planes) and snerf_terrain_fill
 * (four int32 planes) need for an (h, w) raster -- the larger of the two, 16 h w, whatever the radius; -1 (and a message) for
 * h or w < 1 or h * w >= 2^31. */
long long snerf_terrain_workspace_bytes(int h, int w);

/* snerf_terrain_keys: altitudes to keys and the initial flags, one launch.
 *   alt (h, w) f32;  label (h, w) u8 or NULL;  blocked_host: the classes that can never be ground, or NULL -- both or neither;
 *   key (h, w) int32 and flags (h, w) u8: EVERY word is written:  key = the cell's key, or SNERF_TERRAIN_HOLE;  flags = bit 2 on a
 *     hole, | bit 1 where `label` is given and blocked_host[label[c]] != 0, else 0;
 *   stats[3] u64, zeroed by the caller:  [0] cells whose altitude is finite but out of key range,  [1] cells with a non-finite
 *     altitude,  [2] blocked cells.
 * Refused without touching the device: a null alt, key, flags or stats; label without blocked_host or the reverse; h or w < 1;
 * h * w >= 2^31; q not positive and finite, z0 not finite; blocked_host[255] != 0. */
int snerf_terrain_keys(const float* alt, const unsigned char* label, int h, int w, const unsigned char* blocked_host, double z0,
                       double q, int* key, unsigned char* flags, unsigned long long* stats, void* stream);

/* snerf_terrain_open: one level of the filter -- a grey-scale opening of the keys by the (2 radius + 1)^2 square, four launches.
 *   erosion   e[c] = the minimum of the valid key_in over the window round c clipped to the raster, or "none" when the window
 *             holds no valid cell; e is defined at hole cells too;
 *   dilation  o[c] = the maximum of e over the same window, ignoring "none";
 *   key_out[c] = o[c] where key_in[c] is valid, SNERF_TERRAIN_HOLE where it is a hole: the hole set never changes;
 *   with `flags` (or NULL: a plain opening): where key_in[c] is valid and (long long)key_in[c] - key_out[c] > threshold, bit 0 of
 *     flags[c] is set; the other bits, and bit 0 where it was set, stay;
 *   stats[1] u64, zeroed by the caller: the cells whose bit 0 went from 0 to 1;
 *   ws: snerf_terrain_workspace_bytes(h, w) bytes, 4-byte aligned; no word of it is read before the call has written it.
 * The window minimum and maximum are separable: a row pass then a column pass each, every pass van Herk / Gil-Werman over blocks
 * of 2 radius + 1 cells -- the suffix extrema of a block, then the prefix extrema of the next one, combined: a constant number of
 * loads, stores and comparisons per cell whatever the radius (a column pass cuts a block of 64 cells or more into 16 segments that
 * exchange their totals through LDS).  The flag update rides in the last pass.
 * A radius beyond the raster is legal: the window is then the whole raster.
 * Refused without touching the device: a null key_in, key_out, ws or stats; sizes as above; radius outside
 * [1, SNERF_TERRAIN_MAX_RADIUS]; threshold < 0; key_out == key_in. */
int snerf_terrain_open(const int* key_in, int h, int w, int radius, long long threshold, int* key_out, unsigned char* flags, void* ws,
                       unsigned long long* stats, void* stream);

/* snerf_terrain_fill: the terrain under every cell that is not ground, three launches.
 *   key (h, w) int32, flags (h, w) u8: as the entries above leave them;  alt (h, w) f32: the altitudes the keys came from;
 *   dtm, ndsm (h, w) f32, reach (h, w) int32 or NULL: EVERY word is written.
 *   On a ground cell (flags == 0):  dtm = alt (the input's bits), ndsm = +0, reach = 0.
 *   On any other cell, holes included: the nearest ground cell to the W and to the E along the row and to the N and to the S along
 *   the column, each at a distance d >= 1 in cells with a key k.  With b the smallest of the keys found, in fp64 and in the fixed
 *   order W, E, N, S, skipping a direction that finds none:
 *       num += (double)(k - b) / (double)d;   den += 1.0 / (double)d;
 *       t = z0 + q * ((double)b + num / den);   dtm = (float)t;   ndsm = (float)((double)alt - t), NaN where alt is not finite;
 *   reach = the smallest d used.  Plain IEEE operations, none contracted: a numpy restatement gives the same bits, and a level
 *   ground comes back exactly (k - b = 0).  With no ground in any of the four directions: dtm = ndsm = NaN, reach = -1.
 *   stats[3] u64, zeroed by the caller:  [0] ground cells,  [1] filled cells,  [2] unreachable cells.
 *   ws: as snerf_terrain_open.
 * The nearest ground index travels along every row in both directions (a scan over the lanes with a carry) and along every column
 * in both directions (lanes across columns); one pass over the cells combines them: the cost per cell does not grow with the
 * length of a run that is not ground.
 * Refused without touching the device: a null key, flags, alt, dtm, ndsm, ws or stats; sizes as above; q not positive and finite,
 * z0 not finite. */
int snerf_terrain_fill(const int* key, const unsigned char* flags, const float* alt, int h, int w, double z0, double q, float* dtm,
                       float* ndsm, int* reach, void* ws, unsigned long long* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
