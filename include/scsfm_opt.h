/*
 * scsfm_opt.h -- C ABI of libscsfm_opt.so: Adam over every parameter tensor of both nets in ONE launch
 * (scsfm_hip/optim.py; train.py --optimizer hip), as a hand-written HIP kernel for gfx950 (MI355X).  Both moments live
 * in two flat fp32 buffers; a table in device memory holds one record per tensor and a chunk map gives every workgroup
 * one chunk of one tensor.
 *
 * Conventions
 *  - `table`, `chunk_map`, `exp_avg` and `exp_avg_sq` are DEVICE pointers, and so are the pointers inside the table; the
 *    caller owns every buffer; nothing is retained.  Parameters and gradients are contiguous fp32.
 *  - `stream` is a hipStream_t passed as void*; the one launch is enqueued on it, the call neither synchronises nor
 *    allocates, and there are no atomics: two calls on the same inputs give the same bits.
 *  - Return value: 0 on success, SCSFM_ERR_ARG (-1) for a rejected argument (nothing is launched then), otherwise the
 *    hipError_t of the failed launch.
 *  - Rejected, before any pointer is touched: a NULL table, chunk_map, exp_avg or exp_avg_sq; exp_avg or exp_avg_sq
 *    that is not 16-byte aligned; a table or chunk_map that is not 8-byte aligned; n_tensors <= 0; n_chunks <= 0;
 *    beta1 or beta2 outside [0, 1) (a NaN included); an eps that is negative or not finite.  The library cannot see
 *    how long the map in device memory is: that n_chunks IS its length is the caller's to check (scsfm_hip/optim.py
 *    does).  The kernel for its part skips a map entry that names no tensor of the table or a chunk that starts past its
 *    tensor's end, so a wrong map cannot make it leave the tensors the table names.
 *
 * The table: n_tensors records of SCSFM_OPT_RECORD_BYTES (40) bytes, 8-byte aligned, little endian, no padding:
 *      offset  0  float*       param        n fp32, updated in place
 *      offset  8  const float* grad         n fp32, read only (NULL for a tensor without a chunk in the map)
 *      offset 16  int64        state_offset the tensor's first element in exp_avg and exp_avg_sq; a multiple of 4, so
 *                                           that every segment starts on a 16-byte boundary
 *      offset 24  int32        n            elements, > 0
 *      offset 28  float        step_size             fp32(lr / (1 - beta1^step))          computed in double from the
 *      offset 32  float        bias_correction2_sqrt fp32(sqrt(1 - beta2^step))           tensor's OWN step count, as
 *      offset 36  float        weight_decay          fp32(weight_decay)                   torch.optim.Adam does
 *
 * The chunk map: n_chunks pairs of int32 {tensor, chunk}: workgroup i updates elements [chunk * SCSFM_OPT_CHUNK,
 * min(n, (chunk + 1) * SCSFM_OPT_CHUNK)) of tensor `tensor`.  SCSFM_OPT_CHUNK is 2048 elements: 256 threads with two
 * 16-byte accesses (or eight 4-byte ones) per stream each.  A tensor whose gradient is absent gets no entry: its
 * parameter and state are not touched, and its step count is the caller's not to advance.
 *
 * Arithmetic, per element.  Every line is ONE correctly rounded fp32 operation (no contraction into fused
 * multiply-adds; denormals are kept), in exactly this order; with the host-side constants
 *      b1  = (float)beta1    b1c = (float)(1.0 - beta1)    b2 = (float)beta2    b2c = (float)(1.0 - beta2)
 *      e   = (float)eps                                    (1.0 - beta in double, then rounded; b1 itself is unused)
 *
 *      if (weight_decay != 0) { t = weight_decay * p;  g = g + t; }
 *      t = g - m;      t = b1c * t;     m = m + t;
 *      a = v * b2;     t = b2c * g;     t = t * g;      v = a + t;
 *      d = sqrtf(v);   d = d / bias_correction2_sqrt;   d = d + e;
 *      t = m / d;      t = step_size * t;               p = p - t;
 *
 * m, v and p are stored; g is not.  A chunk whose four addresses (p, g, m, v at the chunk's start) are all 16-byte
 * aligned is read and written with 16-byte accesses, any other one with 4-byte accesses (a gradient that is a view into
 * a bucket at an odd element offset); the arithmetic is the same.
 */
#ifndef SCSFM_OPT_H_
#define SCSFM_OPT_H_

#include <stddef.h>

#define SCSFM_OPT_CHUNK 2048
#define SCSFM_OPT_RECORD_BYTES 40

#ifdef __cplusplus
extern "C" {
#endif

/* 1 (first version) */
int scsfm_opt_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: opt_source_id) into buf, NUL-terminated */
int scsfm_opt_source_id(char* buf, size_t n);

/* one Adam step of every tensor that has an entry in the map */
int scsfm_opt_adam_step_f32(const void* table, int n_tensors, const void* chunk_map, int n_chunks, float* exp_avg,
                            float* exp_avg_sq, double beta1, double beta2, double eps, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_OPT_H_ */
