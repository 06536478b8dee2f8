/*
 * scsfm_cast.h -- C ABI of libscsfm_cast.so: ray casting of a fused TSDF volume (include/scsfm_fuse.h) from camera
 * poses -- a depth map, world normals, a colour picture and a headlight-shaded picture per view -- as hand-written HIP
 * kernels for gfx950 (MI355X).
 *
 * Conventions (as include/scsfm_fuse.h)
 *  - All pointers are DEVICE pointers; the caller owns every buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_CAST_ERR_ARG (-1) for a rejected argument (before any pointer is touched),
 *    otherwise the hipError_t of the failed launch.  Every output is stored (overwritten), never accumulated.
 *  - No atomics: a pixel belongs to one thread and a brick's byte to one thread, so results are bit-identical from run
 *    to run.
 *  - Sizes whose products would overflow int are rejected.
 *
 * Volume.  scsfm_fuse.h's, read in place: nx x ny x nz voxels, x fastest, nvox <= 2^29, five fp32 planes of nvox each
 * (tsdf, weight, r, g, b).  Only read.
 *
 * Arithmetic.  fp32 unless stated, one rounding per operation (no fused multiply-add), `/` and sqrtf correctly rounded,
 * denormals kept.  fl() marks a rounding where the nesting alone might not show it.  lerp(a, b, f) is
 * fl(a + fl(f fl(b - a))).
 *
 * View record (16 floats per view): A row-major (a0 .. a8), the centre (c0 c1 c2), fx, fy, cx, cy -- camera to world.
 * scsfm_cast_views rounds each of the 12 doubles of a pose once to fp32 (a pose row is a_i0 a_i1 a_i2 c_i) and takes
 * fx = K[0], fy = K[4], cx = K[2], cy = K[5].  The pixel convention is the integration's (px = int(u + 0.5)): pixel px
 * has u = px exactly.
 *
 * The ray of pixel (px, py).  dx = fl((float(px) - cx) / fx), dy = fl((float(py) - cy) / fy); the world direction is
 * w_i = (a_i0 dx + a_i1 dy) + a_i2; the point at parameter s is p_i(s) = c_i + fl(s w_i).  The direction has z = 1 in
 * the camera's frame, so s is the depth in the sense of 1 / disp.
 *
 * The field at a point p.  Per axis (origin o_i, n_i voxels): g_i = fl(fl(p_i - o_i) / voxel) - 0.5f.  The sample is IN
 * RANGE iff g_i >= 0 && g_i < float(n_i - 1) on all three axes; the test is made on the float, before any conversion (a
 * NaN or a huge value fails it and converts nothing), and an axis with n_i == 1 has no cell: no sample is in range.
 * Then b_i = int(g_i), f_i = g_i - float(b_i); the eight corners are the voxels (b_x + i, b_y + j, b_z + k), i, j, k
 * in {0, 1}.  The sample is VALID iff it is in range and all eight corner weights are >= min_weight.
 *   T    the trilinear value of tsdf: along x, lerp(t_0jk, t_1jk, f_x) for the four x-edges; then y, lerp(e_0k, e_1k,
 *        f_y); then z, lerp(e_0, e_1, f_z).  A colour channel C uses the same formula on its plane.
 *   G    the gradient, from the same eight corners: G_x is the bilinear value (y then z, the same lerps) of the four
 *        differences fl(t_1jk - t_0jk); G_y of the four fl(t_i1k - t_i0k), reduced along x then z; G_z of the four
 *        fl(t_ij1 - t_ij0), reduced along x then y.
 * A sample is INSIDE iff it is valid and T < 0 (the sign rule of scsfm_fuse.h's crossings: 0.0, -0.0 and a NaN are not
 * inside).
 *
 * The march.  The samples are s_k = fl(near + fl(float(k) step)), k = 0 .. n_steps - 1.  The ray's EVENT is the
 * smallest k >= 1 for which samples k-1 and k are both valid and exactly one of them is inside.
 *  - k-1 not inside, k inside: a HIT.
 *      frac   = T_{k-1} / fl(T_{k-1} - T_k)
 *      depth  = fl(s_{k-1} + fl(fl(s_k - s_{k-1}) frac))
 *      colour = lerp(C_{k-1}, C_k, frac) per channel, then scsfm_fuse.h's byte: c = colour >= 0 ? colour : 0 (a NaN
 *               becomes 0), c = c <= 1 ? c : 1, byte = uint8(fl(fl(c 255.0f) + 0.5f))
 *      N      = lerp(G_{k-1}, G_k, frac) per component, len = sqrtf((N_x N_x + N_y N_y) + N_z N_z),
 *      normal = N / len per component, and (0, 0, 0) unless len > 0 (a NaN fails): world axes, towards free space
 *      L      = fl(-((n_x w_x + n_y w_y) + n_z w_z)) / sqrtf((w_x w_x + w_y w_y) + w_z w_z), then as the colour:
 *               L >= 0 ? L : 0, <= 1 ? : 1, shade = uint8(fl(fl(L 255.0f) + 0.5f))
 *    A depth or a normal component that is a NaN (possible only with non-finite values in the volume) is stored as the
 *    quiet NaN 0x7fc00000: the sign an operation leaves on a NaN is not the same on every machine.
 *  - k-1 inside, k not: the ray met the surface from behind and ENDS WITHOUT A HIT.
 *  - no event: no hit.
 * No hit writes depth 0.0f, normal (0, 0, 0), colour (0, 0, 0) and shade 0.
 *
 * The cull.  scsfm_cast_mask writes one byte (0 or 1) per brick of 8 x 8 x 8 voxels (ceil(n_i / 8) bricks an axis, x
 * fastest, the last ones clipped): brick (Bx, By, Bz) is marked iff some voxel with 8 B_i <= coord_i <= 8 B_i + 8 on
 * every axis (nine wide, clipped to the volume: the corners of every cell whose base voxel is in the brick) has
 * weight >= min_weight && tsdf < 0.  With a mask, scsfm_cast_cast fetches the corners only of a sample whose own brick
 * (that of its base voxel), its predecessor's or its successor's is marked; a sample in an unmarked brick cannot be
 * inside and an event needs an inside sample at k-1 or k, so the outputs are the same bits with a mask, with
 * mask == NULL (every sample is evaluated) and with a mask of all ones.  The mask must be scsfm_cast_mask's for the same
 * volume and min_weight, or mark more.
 */
#ifndef SCSFM_CAST_H_
#define SCSFM_CAST_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCSFM_CAST_ERR_ARG (-1)
#define SCSFM_CAST_MAX_VOXELS (1 << 29)
#define SCSFM_CAST_VIEW 16           /* floats per view record */
#define SCSFM_CAST_BRICK 8           /* voxels per brick and axis */
#define SCSFM_CAST_MAX_STEPS (1 << 20)

/* 1 (first version) */
int scsfm_cast_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: cast_source_id) into buf, NUL-terminated */
int scsfm_cast_source_id(char* buf, size_t n);

/* c2w [n, 12] doubles (what scsfm_odom_chain writes: camera to world), K [9] floats (row-major 3 x 3, shared by the
   views) -> view [n, 16].  Rejected: n <= 0, n 16 past int, a NULL pointer. */
int scsfm_cast_views(int n, const double* c2w, const float* K, float* view, void* stream);

/* bytes of the brick mask of a volume of nx x ny x nz voxels (one per brick); 0 for a rejected argument (a size <= 0,
   nvox > 2^29) */
size_t scsfm_cast_mask_bytes(int nx, int ny, int nz);

/* Writes every byte of the brick mask (see above).  Rejected: a size <= 0, nvox > 2^29, a NULL volume or mask, a volume
   not aligned to 4 bytes, min_weight < 1 (or NaN or infinite). */
int scsfm_cast_mask(int nx, int ny, int nz, const float* volume, float min_weight, unsigned char* mask, void* stream);

/* Casts V views of H x W pixels (see above).  view [V, 16]; mask: scsfm_cast_mask's bytes or NULL; depth [V, H, W]
   fp32; normal [V, 3, H, W] fp32; rgb [V, H, W, 3] bytes; shade [V, H, W] bytes.  Each of normal, rgb and shade may be
   NULL and is then neither computed nor written.  Rejected: a size <= 0, nvox > 2^29, V <= 0, H W or V 3 H W past int,
   n_steps < 1 or > 2^20, voxel <= 0, step <= 0, min_weight < 1, near < 0 (or any of them, or the origin, NaN or
   infinite), a NULL volume, view or depth, a volume, view, depth or normal not aligned to 4 bytes. */
int scsfm_cast_cast(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, const float* volume,
                    float min_weight, float near_s, float step, int n_steps, int V, int H, int W, const float* view,
                    const unsigned char* mask, float* depth, float* normal, unsigned char* rgb, unsigned char* shade,
                    void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_CAST_H_ */
