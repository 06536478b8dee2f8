/*
 * scsfm_roll.h -- C ABI of libscsfm_roll.so: a truncated signed distance volume of fixed size that follows the camera
 * (reconstruct.py --follow), as hand-written HIP kernels for gfx950 (MI355X): the shift of the five planes by whole
 * voxels, and the extraction of the surface points that leave with it.
 *
 * Conventions (as include/scsfm_fuse.h)
 *  - All pointers are DEVICE pointers; the caller owns every buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_ROLL_ERR_ARG (-1) for a rejected argument (before any pointer is touched),
 *    otherwise the hipError_t of the failed launch.  Every output is stored (overwritten), never accumulated.
 *  - No float atomics: a voxel of the destination belongs to one thread, and the extracted points are placed by an integer
 *    scan, so results are bit-identical from run to run.
 *
 * Volume.  As include/scsfm_fuse.h: nx x ny x nz voxels, x fastest (voxel (x, y, z) has the linear index (z ny + y) nx + x),
 * any positive sizes with nvox = nx ny nz <= 2^29; five fp32 planes of nvox each, one after another: tsdf, weight, r, g, b.
 * Plane and byte offsets are size_t (five planes of 2^29 floats pass 4 GB).
 *
 * Lattice.  A rolling volume has a fixed origin0 (fp32), a voxel size s and a cumulative integer offset k = (kx, ky, kz) in
 * voxels.  The origin that every kernel of the project is handed (integrate, extract, cast, track, conf, and the extraction
 * below) is, per axis,
 *   o_k = fl(origin0 + fl(float(k) s))                              (fp32, one rounding per operation)
 * recomputed from k every time and never accumulated; the host computes it (scsfm_hip.rolling.origin_at, numpy fp32).  The
 * centre of voxel i stays  fl(o_k + fl(fl(float(i) + 0.5f) s)).  This library itself sees only o_k.
 *
 * Shift.  For all five planes, dst voxel (x, y, z) takes the BITS of src voxel (x + sx, y + sy, z + sz) where that lies
 * inside the volume, and 0.0f (all bits zero) elsewhere: NaNs and denormals pass unchanged.  Out of place: every dst
 * element is written exactly once, every kept src element is read once, src is only read.  Any integer shift is accepted,
 * 0 included (a copy), and |s| >= n on an axis (an all-zero volume).  A thread owns four consecutive floats of dst at a
 * 16-byte boundary of the ADDRESS (whatever nx and the planes' sizes are; the first and last group of a buffer that is
 * only 4-byte aligned are partial), stores them with one 16-byte store and, when its four sources are all inside, loads
 * them with one 16-byte load at their 4-byte alignment: an x-shift that is no multiple of 4 costs nothing else.  The
 * launch has one thread per group, however large the volume.
 *
 * Leaving extraction.  scsfm_roll_count and scsfm_roll_extract are scsfm_fuse_count and scsfm_fuse_extract with a keep
 * box of six ints, [x0, x1) x [y0, y1) x [z0, z1) in voxels.  The crossings, their order, their coordinates and colours
 * are exactly those of include/scsfm_fuse.h ("Extraction"):  the edge from voxel a to its positive neighbour b (inside the
 * volume) on the axes +x, +y, +z, by the linear index of a and then the axis, is a crossing when
 *   w_a >= min_weight && w_b >= min_weight && (t_a < 0) != (t_b < 0),
 *   frac = t_a / fl(t_a - t_b),  the coordinate along the edge's axis fl(c_a + fl(frac voxel)), the other two a's centre,
 *   colour = fl(col_a + fl(frac fl(col_b - col_a))), c = colour >= 0 ? colour : 0 (a NaN becomes 0), c = c <= 1 ? c : 1,
 *   byte = uint8(fl(fl(c 255.0f) + 0.5f)).
 * A crossing is counted and written ONLY IF voxel a or voxel b lies outside the keep box (a voxel is inside when
 * x0 <= x < x1 && y0 <= y < y1 && z0 <= z < z1).  With an empty keep box (x0 >= x1 or y0 >= y1 or z0 >= z1) no voxel is
 * inside, and the workspace, the count, xyz and rgb are bit for bit what libscsfm_fuse.so leaves; the workspace has the
 * same layout and size.  A chunk of SCSFM_ROLL_CHUNK voxels whose voxels and their +x / +y / +z neighbours all lie inside
 * the keep box does not load the volume (its count is stored as 0), and neither does a voxel of another chunk of which
 * that holds: what is read is the leaving slab.
 *
 * Why this rule.  When the window moves by s, the old voxels that survive are i in [max(0, s), min(n, n + s)) per axis:
 * the keep box.  An edge with an end outside it cannot be completed later, so it is emitted now; an edge with both ends
 * kept stays in the volume and is emitted by a later shift or by the final extraction.  Every edge of the world lattice is
 * emitted at most once.
 */
#ifndef SCSFM_ROLL_H_
#define SCSFM_ROLL_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCSFM_ROLL_ERR_ARG (-1)
#define SCSFM_ROLL_MAX_VOXELS (1 << 29)
#define SCSFM_ROLL_PLANES 5      /* tsdf, weight, r, g, b */
#define SCSFM_ROLL_CHUNK 1024    /* consecutive voxels (by linear index) per extraction chunk, as SCSFM_FUSE_CHUNK */

/* 1 (first version) */
int scsfm_roll_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: lib_source_id) into buf, NUL-terminated */
int scsfm_roll_source_id(char* buf, size_t n);

/* dst <- src moved by (sx, sy, sz) voxels (see "Shift").  Rejected: a size <= 0, nvox > 2^29, a NULL src or dst, one not
   aligned to 4 bytes, and dst and src whose 20 nvox bytes overlap (dst == src included). */
int scsfm_roll_shift(int nx, int ny, int nz, int sx, int sy, int sz, const float* src, float* dst, void* stream);

/* bytes of the workspace of scsfm_roll_count and scsfm_roll_extract: scsfm_fuse_extract_ws_bytes' value and layout, in
   ints: [0] the number of crossings, [1 .. 3] unused, the count of every chunk, the exclusive scan of those counts.  0 for
   a rejected argument. */
size_t scsfm_roll_ws_bytes(int nx, int ny, int nz);

/* Counts the leaving crossings of every chunk, scans the counts and stores the total, all into ws (16-byte aligned,
   ws_bytes >= scsfm_roll_ws_bytes).  min_weight >= 1.  The keep box may be any six ints. */
int scsfm_roll_count(int nx, int ny, int nz, int x0, int x1, int y0, int y1, int z0, int z1, const float* volume,
                     float min_weight, void* ws, size_t ws_bytes, void* stream);

/* Writes the leaving crossings in their order: point k < capacity to xyz[k, 3] and rgb[k, 3]; nothing at or past
   capacity.  ws is what scsfm_roll_count left for the same volume, keep box and min_weight; (ox, oy, oz) is o_k.
   capacity >= 0 (0: xyz and rgb may be NULL). */
int scsfm_roll_extract(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, int x0, int x1, int y0, int y1,
                       int z0, int z1, const float* volume, float min_weight, const void* ws, size_t ws_bytes,
                       int capacity, float* xyz, unsigned char* rgb, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_ROLL_H_ */
