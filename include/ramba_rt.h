/* ramba_rt — C-ABI runtime for the MI355X-native Ramba hot-path backend.
 *
 * This is the drop-in boundary of SURVEY.md §8(b): the Python host lowers
 * each fused deferred-op group (the payload of the reference's
 * remote_exec_all("run_deferred_ops", ...) call, ramba/ramba.py:8286-8298)
 * to generated gfx950 HIP source + a packed argument buffer, and drives it
 * through these entry points.  No torch types cross this boundary — only
 * plain pointers and sizes.
 *
 * Reference interfaces each entry point replaces (file:line in the
 * reference repo Python-for-HPC/ramba):
 *   rt_init           — worker startup / device binding (ramba.py:10646-10725)
 *   rt_kernel_get     — FunctionMetadata JIT + sha-keyed code cache
 *                       (ramba.py:249-438, fname hash at 8260)
 *   rt_launch         — the fused-loop invocation func(global_start,
 *                       itershape, ...) (ramba.py:3768/3779)
 *   rt_copy_box       — shard sub-box pack/unpack for the part/halo
 *                       exchange (comm_queues puts at ramba.py:3656,
 *                       getborder ramba.py:1260) and gather (get_view 2160)
 *   rt_take_rows      — indexed row gather for a[int_array] / take
 *                       (all2all getitem worker, ramba.py:3960)
 *   rt_gemm           — the local np.dot of the matmul workers
 *                       (ramba.py:3056, 6953-7040), on the MFMA units
 *   rt_gemm_batched   — the same for N-D (batched) operands
 *   rt_gemv           — the same for one 1-D operand (A @ x, x @ A)
 *   rt_hist           — histogram / bincount (no reference counterpart)
 *   rt_sort           — stable radix sort of a dense run, optional payload
 *   rt_sort_lines     — stable sort of many short lines (sort / argsort
 *                       along an axis; no reference counterpart)
 *   rt_sort_bounds    — lower bounds of splitter keys in a sorted run
 *   rt_select_pass    — one counting pass of a radix select (median /
 *                       percentile / quantile; no reference counterpart)
 *   rt_unique_count /
 *   rt_unique_write   — run compaction of a sorted run (unique; no reference
 *                       counterpart)
 *   rt_searchsorted   — batched binary search behind an LDS fence
 *                       (searchsorted; no reference counterpart)
 *   rt_partition      — stable multi-pivot split of a dense run (partition /
 *                       argpartition; no reference counterpart)
 *   rt_stream_sync /
 *   rt_device_sync    — worker-side completion (sync, ramba.py:9843)
 *   rt_event_*        — hot-loop timing (add_time, ramba.py:945-1022)
 *
 * Python-side binding: the ctypes table in ramba_amd/hip_backend.py
 * (_load_lib); see INTEGRATION.md.
 */

#ifndef RAMBA_RT_H
#define RAMBA_RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* All functions return 0 on success, nonzero on failure; rt_last_error()
 * returns a static string describing the last failure (fail-fast contract —
 * the analog of the reference's ("ERROR", worker, traceback) reply,
 * ramba.py:3878-3881). */

/* Element-type codes of every `int dtype` parameter below.  This is the one
 * statement of the list: the runtime dispatches on these names and the
 * Python binding's RT_DTYPE table mirrors them.
 *   RT_F64 double   RT_F32 float    RT_I64 int64_t   RT_I32 int32_t
 *   RT_I16 int16_t  RT_I8  int8_t   RT_U8  uint8_t (also bool)
 * rt_cumsum and rt_axis_scan take the first four (RT_F64 .. RT_I32);
 * rt_combine_box, rt_mask_compact and the rt_arg_* family take all seven.
 * Any other value is rejected with "<entry>: bad dtype". */
enum rt_dtype { RT_F64 = 0, RT_F32, RT_I64, RT_I32, RT_I16, RT_I8, RT_U8 };

int         rt_init(int device);
int         rt_device_count(void);
const char *rt_last_error(void);

/* Compile (hiprtc, gfx950) and cache a kernel. `key` is the host-computed
 * structural hash of the fused group (the analog of the sha256 code hash at
 * ramba.py:8260); `source` is full HIP source; `kname` the extern-C kernel
 * symbol.  Returns a handle valid for the process lifetime. */
int rt_kernel_get(const char *key, const char *source, const char *kname,
                  void **out_kernel);

/* Compile-only validation of generated source (no GPU needed). */
int rt_compile_check(const char *source);

/* Launch a compiled kernel with a packed argument buffer (passed via
 * HIP_LAUNCH_PARAM_BUFFER_POINTER).  block is (bx,1,1). */
int rt_launch(void *kernel, unsigned gx, unsigned gy, unsigned gz,
              unsigned bx, uintptr_t stream, const void *args,
              size_t argsize);

/* Argument contract shared by rt_copy_box, rt_combine_box, rt_cumsum,
 * rt_mask_compact, rt_axis_scan, rt_flat_copy, rt_hist, rt_partition and the
 * rt_sort family (the contract of
 * rt_take_rows): every argument is checked on the host before any HIP call
 * and a bad one returns nonzero with rt_last_error() naming the entry point
 * and the argument.  Rejected: nd out of range; NULL shape / strides; a
 * negative extent; an extent of 2^40 or more or an extent product above
 * 2^46 (the rt_arg_* limits); a dtype / elemsize / op / phase / scatter
 * code outside the listed values; a NULL data pointer when there is work to
 * do.  A zero extent returns 0 without launching.  Offsets and strides are
 * NOT checked against the allocations (the entry points do not know their
 * sizes): keeping the box inside both buffers is the caller's job. */

/* Strided box copy between device buffers (pack/unpack/halo/gather).
 * shape/strides are in elements, 1 <= nd <= 4, elemsize in {1,2,4,8}.
 * One thread per element, at most 2048 blocks of 256 (grid-stride). */
int rt_copy_box(uintptr_t stream, void *dst, const void *src, int nd,
                const int64_t *shape, const int64_t *dst_strides,
                const int64_t *src_strides, int64_t dst_off, int64_t src_off,
                int elemsize);

/* Typed combining box copy: dst = dst OP src (axis-reduction merge).
 * dtype: any rt_dtype;
 * op: 0=add 1=mul 2=min 3=max 4=logical_and 5=logical_or.  Float min/max
 * propagate NaN from either side; the logical ops write 0 or 1. */
int rt_combine_box(uintptr_t stream, void *dst, const void *src, int nd,
                   const int64_t *shape, const int64_t *dst_strides,
                   const int64_t *src_strides, int64_t dst_off,
                   int64_t src_off, int dtype, int op);

/* Elements per chunk of the rt_cumsum phases (one bsums slot each) and of
 * rt_mask_compact (one bcounts slot each).  Host arithmetic only. */
int rt_scan_chunk(void);
int rt_mask_chunk(void);

/* cumsum phases (local scan; cross-rank offset fixed up by the host):
 * phase 1: chunk sums into `bsums[ceil(n / rt_scan_chunk())]`; phase 2:
 * one-block exclusive scan of bsums[0, nblocks) in place + grand total into
 * `total` (may be NULL); phase 3: apply with `fbase`/`ibase` (the rank's
 * global offset).  In phases 1 and 3 `nblocks` is the launch grid: the
 * blocks stride over the chunks of n, so any value >= 1 is valid.
 * dtype: RT_F64 .. RT_I32; phase: 1, 2 or 3, anything else is
 * rejected.  Needed pointers: in + bsums (1), bsums (2), in + out + bsums
 * (3).  n == 0 returns 0 without launching in phases 1 and 3; phase 2
 * ignores in / n / out. */
int rt_cumsum(uintptr_t stream, const void *in, int64_t in_off,
              int64_t in_stride, int64_t n, void *out, int64_t out_off,
              void *bsums, int64_t nblocks, void *total, double fbase,
              int64_t ibase, int dtype, int phase);

/* Ordered boolean-mask compaction over the rank's local core box, C
 * iteration order (reference: the compressing boolean getitem of
 * ramba.ndarray, ramba/ramba.py maskarray path).  phase 1: selected counts
 * per chunk of rt_mask_chunk() (2048) elements into bcounts
 * (int64[nchunks]); phase 2 is rt_cumsum(phase=2, dtype=RT_I64) on bcounts
 * (exclusive scan + total); phase 3: write selected elements of `a` densely
 * into `out`.  nchunks must equal ceil(n / rt_mask_chunk()), n the extent
 * product.  The mask is one byte per element, nonzero = selected; its
 * counts are read 8 bytes at a time when it is 1-D, stride 1 and 8-byte
 * aligned.  dtype: any rt_dtype; phase 1 or 3.
 * Needed pointers: m + bcounts (1); a + m + out + bcounts (3). */
int rt_mask_compact(uintptr_t stream, const void *a, const void *m,
                    void *out, int nd, const int64_t *shape,
                    const int64_t *a_strides, const int64_t *m_strides,
                    void *bcounts, int64_t nchunks, int dtype, int phase);

/* Inclusive cumulative sum along `axis` of a strided box (the N-D half of
 * the reference's scumulative, ramba/ramba.py:10057-10171).  in / out are
 * pre-offset to the box origin; shape and both stride lists cover the full
 * box, 2 <= nd <= 4, strides in elements.  totals: dense C-order array over
 * the box with `axis` removed; receives each line's sum (its last scanned
 * element).  dtype: RT_F64 .. RT_I32.
 * nchunks == 1: one wave per line when axis == nd-1, else one thread per
 * line.  nchunks > 1: the axis is cut into nchunks ranges of
 * ceil(len / nchunks), one thread per (line, range), with tot2
 * (nchunks * nlines elements of the dtype) as scratch; trailing ranges may
 * be empty.  nchunks < 1, or nchunks > 1 with tot2 == NULL, is rejected. */
int rt_axis_scan(uintptr_t stream, const void *in, void *out, void *totals,
                 int nd, const int64_t *shape, const int64_t *in_strides,
                 const int64_t *out_strides, int axis, int dtype, void *tot2,
                 int64_t nchunks);

/* Flat C-order gather (scatter=0) / scatter (scatter=1) between a strided
 * local box and a dense buffer — the data movement of reshape (reference
 * flat-index remap worker, ramba/ramba.py:2409-2492).  `boxed` is
 * pre-offset to the box origin; [flat0, flat0 + n) is a C-order flat
 * subrange of the box and must lie inside it (flat0 >= 0, n >= 0,
 * flat0 + n <= extent product).  elemsize in {1,2,4,8}. */
int rt_flat_copy(uintptr_t stream, void *boxed, void *dense, int nd,
                 const int64_t *shape, const int64_t *strides,
                 int64_t flat0, int64_t n, int elemsize, int scatter);

/* Indexed row gather / placement — the data movement of integer-array
 * getitem and take() (reference all2all getitem worker,
 * ramba/ramba.py:3960, getitem 6443-6545):
 *     dst[dr(k)] = src[sr(k)]   for k in [0, n)
 * where a "row" is a strided box of up to 3 inner axes; sr(k) =
 * src_rows ? src_rows[k] : k, likewise dr(k).  A source row in
 * [-src_nrows, 0) wraps once (NumPy negative index).  dst/src point at row
 * 0; strides are in elements; src_rows/dst_rows are device int64[n].
 * elemsize in {1,2,4,8}.  Rows outside [0,src_nrows) / [0,dst_nrows) are
 * skipped and counted in *bad (device uint32, may be NULL).  Arguments are
 * validated before any HIP call; n == 0 returns 0 without launching. */
int rt_take_rows(uintptr_t stream, void *dst, const void *src,
                 const int64_t *src_rows, const int64_t *dst_rows, int64_t n,
                 int64_t src_nrows, int64_t dst_nrows, int nd_inner,
                 const int64_t *inner_shape, const int64_t *src_strides,
                 const int64_t *dst_strides, int64_t src_row_stride,
                 int64_t dst_row_stride, int elemsize, void *bad);

/* The kernel rt_take_rows picks for a geometry: 0 = narrow (one thread per
 * element, rows under 256 B), 1 = wide (one wave per row) with 16-byte
 * accesses, 2 = wide scalar; -1 on invalid arguments.  Host arithmetic
 * only. */
int rt_take_regime(const void *dst, const void *src, int nd_inner,
                   const int64_t *inner_shape, const int64_t *src_strides,
                   const int64_t *dst_strides, int64_t src_row_stride,
                   int64_t dst_row_stride, int elemsize);

/* argmax / argmin / nanargmax / nanargmin — (value, index) pair reductions
 * (the reference lists them as to-do, ramba/ramba.py:10288).  One pass over
 * a strided box of 1..4 axes at `in + in_off` (offset and strides in
 * elements); every merge uses rt_arg_better (include/ramba_argcmp.h).
 * dtype: any rt_dtype (bool is RT_U8).  Reported indices
 * are idx0 + sum_d coord_d * mult_d; -1 = no candidate (skipna, all NaN).
 * mult must make the index grow with C order over the box (the C strides
 * of an enclosing shape, or 1 on the reduced axis): threads rely on it.
 * nd, extents (>= 1), the dtype code and pointers are validated before any
 * launch; a bad argument returns nonzero.
 *
 * rt_arg_flat: all axes -> out_val[1], out_idx[1] (device).  scratch_vals /
 * scratch_idx hold rt_arg_grid_cap() pairs (8 bytes each side per pair).
 * Stage 1 runs at most rt_arg_grid_cap() blocks of 256 lanes, each lane
 * taking one load unit per trip, two trips per loop pass; a unit is 16
 * bytes when rt_arg_flat_regime() is 1, else one element.
 *
 * rt_arg_axis: one axis -> out_vals / out_idx, dense C order over the kept
 * axes; mult is 1 on `axis`.  axis == nd-1: one wave per line (16-byte
 * loads when the axis stride is 1 and every line is aligned).  Otherwise
 * one thread per output element, or, with nchunks > 1, per (chunk, output)
 * into part_vals / part_idx [nchunks * nout] followed by a pair reduce.
 *
 * rt_arg_combine_box: dst(val, idx) = better(dst, src) over a box; the
 * destination value and index arrays have their own strides and offsets. */
int rt_arg_grid_cap(void);
int rt_arg_flat_regime(const void *in, int64_t in_off, int nd,
                       const int64_t *shape, const int64_t *strides,
                       int dtype);
int rt_arg_flat(uintptr_t stream, const void *in, int64_t in_off, int nd,
                const int64_t *shape, const int64_t *strides,
                const int64_t *mult, int64_t idx0, int dtype, int is_max,
                int skipna, void *scratch_vals, void *scratch_idx,
                void *out_val, void *out_idx);
int rt_arg_axis(uintptr_t stream, const void *in, int64_t in_off, int nd,
                const int64_t *shape, const int64_t *strides, int axis,
                int64_t idx0, int dtype, int is_max, int skipna,
                int64_t nchunks, void *part_vals, void *part_idx,
                void *out_vals, void *out_idx);
int rt_arg_combine_box(uintptr_t stream, void *dst_vals, void *dst_idx,
                       const void *src_vals, const void *src_idx, int nd,
                       const int64_t *shape, const int64_t *dst_val_strides,
                       const int64_t *dst_idx_strides,
                       const int64_t *src_strides, int64_t dst_val_off,
                       int64_t dst_idx_off, int dtype, int is_max,
                       int skipna);

/* Dense GEMM on the matrix units: C[M,N] (+)= A[M,K] @ B[K,N] — the local
 * np.dot of the reference's matmul workers (ramba/ramba.py:3056,
 * 6953-7040).  c / a / b point at element (0,0); strides are in elements;
 * C has column stride 1 and row stride ldc >= N.  dtype: RT_F64
 * (v_mfma_f64_16x16x4) or RT_F32 (v_mfma_f32_32x32x2).  accumulate: 0
 * overwrites C, 1 adds to what it holds.  One 256-lane block per
 * rt_gemm_tile() tile of C; M, N, K need not be multiples of it, and
 * nothing outside the three matrices is read or written.  A with a_cs == 1
 * and B with b_cs == 1 are read with 16-byte loads when base and row stride
 * are 16-byte aligned; every other stride pattern (transposed, odd leading
 * dimension, odd column offset) is read element-wise.  Each output element
 * is summed in ascending k by one wave: no atomics, same bits every run.
 * Validated before any HIP call: negative extents, extents >= 2^40, M*N,
 * M*K or K*N above 2^46, ldc < N, dtype, accumulate, NULL pointers with
 * work to do.  M == 0 or N == 0 returns 0 without launching; K == 0
 * zero-fills C (accumulate 0) or leaves it (accumulate 1).
 * rt_gemm_tile: the block tile compiled in for `dtype`; host arithmetic. */
int rt_gemm(uintptr_t stream, void *c, const void *a, const void *b,
            int64_t M, int64_t N, int64_t K, int64_t a_rs, int64_t a_cs,
            int64_t b_rs, int64_t b_cs, int64_t ldc, int dtype,
            int accumulate);
int rt_gemm_tile(int dtype, int *bm, int *bn, int *bk);

/* A batch of GEMMs in one launch: for i in [0, batch),
 * C_i[M,N] (+)= A_i[M,K] @ B_i[K,N] with X_i = x + i * x_bs (batch strides
 * in elements).  a_bs or b_bs may be 0: that operand is shared by every
 * entry.  c_bs must be at least (M-1)*ldc + N when batch > 1, so the
 * results cannot overlap.  The kernel, the tile and every rule of rt_gemm
 * hold (rt_gemm is the batch == 1 call of the same launch path); blocks walk
 * batch x tiles tile indices, batch-major.  An operand takes 16-byte loads
 * only if its batch stride is 16-byte aligned too.  Validated in addition:
 * negative batch, batch >= 2^40, batch*M*N, batch*M*K or batch*K*N above
 * 2^46 (shared operands included), c_bs.  batch == 0 returns 0 without
 * launching. */
int rt_gemm_batched(uintptr_t stream, void *c, const void *a, const void *b,
                    int64_t batch, int64_t M, int64_t N, int64_t K,
                    int64_t a_rs, int64_t a_cs, int64_t b_rs, int64_t b_cs,
                    int64_t ldc, int64_t a_bs, int64_t b_bs, int64_t c_bs,
                    int dtype, int accumulate);

/* Matrix-vector product y[M] (+)= A[M,K] @ x[K], RT_F32 or RT_F64 — the
 * 1-D operand forms of the reference's matmul (ramba/ramba.py:6953-7040).
 * y / a / x point at element 0; all strides are in elements and arbitrary;
 * x @ A is the same call on A's transposed strides.  The kernel ("regime")
 * follows A's unit stride so that A is read once, coalesced:
 *   0 ROW_VEC   a_cs == 1, base and a_rs 16-byte aligned: a wave per 4 rows,
 *               lanes walk k with 16-byte loads, shuffle-tree reduction
 *   1 ROW_ELEM  a_cs == 1 otherwise: the same with element loads
 *   2 COL_VEC   a_rs == 1, base and a_cs 16-byte aligned: lanes along m,
 *               16 bytes (VEC outputs) per thread, VEC thread groups
 *               interleaved over k and summed through LDS in group order
 *   3 COL_ELEM  anything else: one output per thread, general strides
 * A block stages k_step elements of x in LDS and shares them among its
 * rows_per_block outputs (rt_gemv_geometry; host arithmetic).
 * ksplit >= 1 cuts K into ksplit ranges of ceil(K / ksplit) rounded up to
 * k_step (trailing ranges may be empty and are not launched); with
 * ksplit > 1 the blocks write partial sums to scratch (ksplit * M elements
 * of the dtype, caller-owned) and a second kernel adds the ranges in
 * ascending order.  No atomics: (shape, strides, ksplit) fixes the bits.
 * accumulate: 0 overwrites y, 1 adds to it.  Nothing outside A, x, y and
 * scratch is touched; lanes past an edge skip the multiply.
 * Validated before any HIP call: dtype, negative extents, extents >= 2^40,
 * M*K above 2^46, accumulate, ksplit < 1 or > 4096, ksplit > 1 with NULL
 * scratch, NULL y / a / x with work to do.  M == 0 returns 0 without
 * launching; K == 0 zero-fills y (accumulate 0) or leaves it (1).
 * rt_gemv_plan: the regime rt_gemv will take for these arguments and the
 * ksplit to pass: above 1 when the row blocks alone give a chip of `cus`
 * compute units fewer than 4 blocks each, as far as every range keeps two
 * k steps.  Host arithmetic; `cus` is an argument so that it stays so. */
int rt_gemv(uintptr_t stream, void *y, const void *a, const void *x,
            int64_t M, int64_t K, int64_t a_rs, int64_t a_cs, int64_t x_s,
            int64_t y_s, int dtype, int accumulate, int64_t ksplit,
            void *scratch);
int rt_gemv_geometry(int dtype, int regime, int *rows_per_block, int *k_step);
int rt_gemv_plan(const void *a, int64_t M, int64_t K, int64_t a_rs,
                 int64_t a_cs, int dtype, int cus, int *regime,
                 int64_t *ksplit);

/* histogram / bincount — a keyed count (numpy.histogram, numpy.bincount; the
 * reference has neither).  One pass over a strided box of 1..4 axes at
 * `in + in_off` (offset and strides in elements, any sign, zero allowed),
 * binned as if flattened; the kernel ADDS into counts, a device
 * int64[nbins] that the caller zeroes.  dtype: any rt_dtype.
 * mode:
 *   0 INDEX    integer dtypes and RT_U8: the bin is the value; values < 0 or
 *              >= nbins are skipped and counted in *bad (device uint32, may
 *              be NULL).  Nothing outside counts is ever written.
 *   1 UNIFORM  edges: device array of nbins + 1 values, edges_dtype RT_F32
 *              or RT_F64.  NumPy's index computation in that dtype: drop x
 *              unless first <= x <= last (NaN fails); convert x; f = ((x -
 *              first) / (last - first)) * nbins with one IEEE divide and one
 *              IEEE multiply; truncate; nbins becomes nbins - 1; one step
 *              down if x < edges[i], else one up if x >= edges[i+1] and i is
 *              not the last bin.
 *   2 EDGES    any non-decreasing edges, RT_F64: x goes to bin i iff
 *              edges[i] <= x < edges[i+1] (last bin closed), by binary
 *              search, compared in float64; NaN and values outside are
 *              dropped.
 * Range tests and the EDGES search compare in float64, so int64 values above
 * 2^53 are binned by their rounded value.  Edge lists of at most
 * edges_lds_max values are staged in LDS, longer ones are read in place.
 * Counters by nbins (rt_hist_regime): 0 LDS_WAVE, nbins <= wave_max_bins, a
 * private uint32 LDS copy per wave of the 256-lane block; 1 LDS_BLOCK,
 * nbins <= block_max_bins, one uint32 LDS copy per block; 2 GLOBAL, 64-bit
 * atomic adds on counts.  A block adds its nonzero LDS bins to counts with
 * 64-bit atomic adds (integers: the counts do not depend on the order); at
 * most grid_cap blocks run, and no block counts more than 2^31 elements
 * between flushes.  Only when every active lane of a wave holds the same bin
 * does one lane add the lane count; any other mix adds lane by lane.
 * 16-byte loads under the rt_arg_flat_regime rule, else element loads.
 * Validated before any HIP call (the contract above): nd, NULL shape /
 * strides, extents, dtype, mode, INDEX with a float dtype, nbins < 1 or
 * >= 2^40, NULL edges or a bad edges_dtype in modes 1 and 2, NULL in /
 * counts with work to do.  A zero extent returns 0 without launching.
 * rt_hist_regime: the regime for nbins, -1 if nbins is invalid.
 * rt_hist_geometry: the compiled-in constants (any pointer may be NULL).
 * Both are host arithmetic only. */
int rt_hist(uintptr_t stream, const void *in, int64_t in_off, int nd,
            const int64_t *shape, const int64_t *strides, int dtype, int mode,
            const void *edges, int edges_dtype, int64_t nbins, void *counts,
            void *bad);
int rt_hist_regime(int64_t nbins);
int rt_hist_geometry(int *grid_cap, int *block, int64_t *wave_max_bins,
                     int64_t *block_max_bins, int64_t *edges_lds_max);

/* sort / argsort — numpy.sort / numpy.argsort with kind="stable" (the
 * reference has neither).  The order is defined ONCE, in ramba_sortkey.h:
 * every digit and comparison reads rt_sort_canon(raw bits) (integers by
 * value; floats -inf < .. < -0.0 == +0.0 < .. < +inf < NaN, all NaNs equal),
 * ties go to the lower position, and the kernels move the raw bits, so zero
 * signs and NaN payloads arrive as they were.  dtype: any rt_dtype.
 *
 * rt_sort, the LONG regime: a dense run of n keys at `in` sorted into `out`,
 * a stable LSD radix sort with 8-bit digits, one pass per key byte.  With
 * vals_out != NULL every key carries an int64 payload, read from vals_in or,
 * when vals_in is NULL, generated as val0 + position; the sorted payloads
 * land in vals_out (vals_in = NULL, val0 = 0 is argsort).  With vals_out ==
 * NULL the payload is dropped and vals_in is not read.  One up-front read
 * builds the histogram of every digit position; the host reads it back (the
 * call synchronises the stream once) and skips each pass whose digit is the
 * same in all n keys; *passes_run (may be NULL) is how many ran.  A live
 * pass is three launches: per-block digit counts, one scan block per digit,
 * scatter.  No kernel waits for another block.  Passes ping-pong between out
 * and the scratch so that the last one writes out (and vals_out); with no
 * live pass the run is copied.  `in` / vals_in are only read and must not
 * overlap out, vals_out or the scratch.  At most grid_cap blocks run, each
 * over a contiguous range of tiles of block x keys_per_lane keys.
 * scratch: device memory, 16-byte aligned, of at least rt_sort_scratch(n,
 * dtype, vals_out != NULL) bytes: 16 KB of histograms, 12 bytes per digit
 * and block of counters (at most 6 MB), and one copy of the keys (and of the
 * payloads).
 * Validated before any HIP call: dtype, n < 0 or >= 2^40, NULL in / out /
 * scratch with work to do, a misaligned or too small scratch.  n == 0
 * returns 0 without launching.
 *
 * rt_sort_lines: nlines independent lines of len <= line_max elements of a
 * strided box (line l, element e at in + in_off + l * line_stride + e *
 * elem_stride, in elements, any sign), sorted into dense C-order
 * out_keys[nlines][len] (raw keys), out_pos[nlines][len] (int64 positions
 * 0 .. len-1, argsort), or both; either may be NULL.  Regimes: WAVE, len <=
 * wave_max (64): one line per wave, four per block, a bitonic network in
 * registers on the composite (canonical key, position); BLOCK, len <=
 * line_max: one line per block, the same network in LDS.  The composite is a
 * total order, so the network is stable; padding sorts after every element,
 * NaN included, and is never written.  More than lines_per_launch lines take
 * several launches.
 * Validated before any HIP call: dtype, negative nlines / len, nlines >=
 * 2^40, len > line_max, nlines x len > 2^46, NULL in, both outputs NULL.  A
 * zero extent returns 0 without launching.
 *
 * rt_sort_bounds: for m splitter keys (device, raw bits of `dtype`) the
 * lower bound of each in the sorted run of n keys, in the canonical order:
 * bounds[i] (device int64) = the number of keys that sort strictly before
 * splitters[i].  One thread per splitter, a binary search.  Validated before
 * any HIP call: dtype, n, m < 0 or >= 2^31, NULL pointers with work to do;
 * m == 0 returns 0.
 *
 * rt_sort_scratch (-1 for a bad n or dtype) and rt_sort_geometry (the
 * compiled-in constants; line_max: 4 values, for key widths 1, 2, 4 and 8
 * bytes; any pointer may be NULL) are host arithmetic only. */
int rt_sort(uintptr_t stream, const void *in, void *out, const void *vals_in,
            int64_t val0, void *vals_out, int64_t n, int dtype, void *scratch,
            int64_t scratch_bytes, int *passes_run);
int64_t rt_sort_scratch(int64_t n, int dtype, int with_payload);
int rt_sort_lines(uintptr_t stream, const void *in, int64_t in_off,
                  int64_t nlines, int64_t len, int64_t line_stride,
                  int64_t elem_stride, int dtype, void *out_keys,
                  void *out_pos);
int rt_sort_bounds(uintptr_t stream, const void *run, int64_t n, int dtype,
                   const void *splitters, int64_t m, void *bounds);
int rt_sort_geometry(int *block, int *keys_per_lane, int *grid_cap,
                     int *wave_max, int64_t *lines_per_launch,
                     int64_t *line_max);

/* order statistics — one MSD pass of a radix select (numpy.median /
 * percentile / quantile; the reference has none).  The order is that of
 * ramba_sortkey.h: digits are SELECT_DIGIT_BITS = 8 bits of rt_sort_canon(raw
 * bits), and a selected key is turned back into an element by
 * rt_sort_decode, so no raw element is carried.
 *
 * rt_select_pass reads a strided box of 1..4 axes at `in + in_off`, addressed
 * as rt_hist addresses its input (offset and strides in elements, any sign,
 * zero allowed); dtype: any rt_dtype.
 *   shift       the bit position of this pass's digit: a multiple of 8 with
 *               shift + 8 <= the key width.
 *   nq          1 <= nq <= nq_max (8) prefixes.
 *   prefixes    host array of nq DISTINCT uint64 values: the key bits above
 *               shift + 8 that are already decided, in place (every bit at or
 *               below shift + 8 clear).  On the top pass shift + 8 is the key
 *               width and the one prefix is 0.
 *   counts      device int64[nq][256]; the kernel ADDS, the caller zeroes.
 *               An element whose key matches prefix q above shift + 8 adds
 *               one to counts[q][(key >> shift) & 255]; prefixes are
 *               distinct, so at most one matches.
 *   nan_count   device int64, may be NULL: for float dtypes the kernel adds
 *               the number of elements whose key is all ones (NaN).  It looks
 *               at every element, whatever the prefixes; not counted with
 *               `canonical` set.
 *   collect_buf device array of collect_cap keys (the unsigned type of the
 *   collect_cap dtype's width), may be NULL; cursor: device uint64, zeroed by
 *   cursor      the caller.  Every matching element's canonical key is
 *               appended: a wave stages its matches in LDS (ballot, popcount,
 *               rank among the matching lanes) and appends up to 256 at a
 *               time with one atomic add on the cursor.  Nothing is written
 *               at or past collect_cap; the cursor still counts what did not
 *               fit.  The order of the collected keys is unspecified.
 *   canonical   nonzero: `in` already holds canonical keys of the unsigned
 *               type of dtype's width (a collect buffer), a dense 1-D run;
 *               the transform is skipped.  dtype still names the element type
 *               the keys came from, which fixes the key width, so the one
 *               dtype table needs no unsigned codes.
 * Counters: a private uint32[nq][256] LDS copy per wave of the 256-lane block
 * (32 KB at nq = 8; collecting adds 256 keys of stage per wave, at most 8 KB),
 * flushed with 64-bit atomic adds of the nonzero bins;
 * at most grid_cap blocks run and no block counts more than 2^31 elements
 * between flushes (longer boxes take several launches), both as rt_hist.
 * When every active lane of a wave holds the same (prefix, digit), one lane
 * adds the lane count; when none matches nothing is added.  Prefixes travel
 * as kernel arguments.  16-byte loads under the rt_arg_flat_regime rule, else
 * element loads.  counts and nan_count are exact integers, so every result is
 * the same from run to run; no kernel waits for another block.
 * Validated before any HIP call: nd, NULL shape / strides, extents, dtype,
 * shift, nq, NULL / out-of-place / duplicate prefixes, collect_cap < 0, a
 * collect buffer without a cursor, canonical with nd != 1 or a non-unit
 * stride, NULL in / counts with work to do.  A zero extent returns 0 without
 * launching.
 * rt_select_geometry: the compiled-in constants (any pointer may be NULL);
 * host arithmetic only. */
int rt_select_pass(uintptr_t stream, const void *in, int64_t in_off, int nd,
                   const int64_t *shape, const int64_t *strides, int dtype,
                   int canonical, int shift, int nq, const uint64_t *prefixes,
                   void *counts, void *nan_count, void *collect_buf,
                   int64_t collect_cap, void *cursor);
int rt_select_geometry(int *grid_cap, int *block, int *nq_max,
                       int *digit_bits);

/* unique — numpy.unique of a SORTED dense run (the reference has none): the
 * run compaction that follows rt_sort.  keys: n raw keys of `dtype` (any
 * rt_dtype) in the canonical order of ramba_sortkey.h, as rt_sort leaves
 * them; pos: optionally the n int64 payloads that travelled with them (the
 * global positions of a stable argsort).
 *
 * Head rule, the only test of equality: key i is a run head iff i == 0 or
 * rt_sort_canon(key[i]) != rt_sort_canon(key[i-1]).  So -0.0 and +0.0 are one
 * value and all NaNs are one value (NumPy's equal_nan=True), and a run's
 * head is its first key in the stable order.
 *
 * Three launches and a small tail, none of which waits for another block, no
 * atomics: every output is the same from run to run.
 *   rt_unique_count   (1) at most grid_cap blocks, each over a contiguous
 *       range of tiles of block x keys_per_lane keys; a lane owns
 *       keys_per_lane CONSECUTIVE keys, read with 16-byte loads when the run
 *       is 16-byte aligned and the tile whole (else by element), and
 *       compares them in registers; the neighbour across a lane boundary
 *       comes by shuffle, the one across a wave or tile boundary from a
 *       second load.  Heads are counted by ballot and popcount; one int64 per
 *       block goes to the scratch.  (2) one block scans the per-block counts.
 *       The call synchronises the stream once and returns the number of
 *       distinct values in *n_unique, so the caller can size the outputs.
 *   rt_unique_write   (3) the same tiling re-flags the heads; a head's slot
 *       u is the block's base from (2), plus the heads of the tiles before,
 *       plus a 4-entry LDS scan over the waves, plus ballot and popcount
 *       within the wave.  Must follow rt_unique_count on the same keys, n and
 *       scratch.  The head at run position i writes
 *           out_keys[u]   = key[i], the RAW bits: the zero sign and the NaN
 *                           payload of the first occurrence survive;
 *           out_first[u]  = pos[i], or i when pos is NULL;
 *           out_counts[u] = i, and two trailing launches turn these starts
 *                           in place into counts[u] = start[u+1] - start[u],
 *                           with n closing the last run.
 *       Each output may be NULL (not all three); a NULL output's stores, and
 *       for out_counts the trailing launches, are skipped.  The call does not
 *       synchronise.
 * scratch: device memory, 16-byte aligned, at least rt_unique_scratch(n)
 * bytes (a few KB: two int64 per block and grid_cap range edges).
 * Validated before any HIP call: dtype, n < 0 or >= 2^40, NULL keys / scratch
 * / n_unique with work to do, a misaligned or too small scratch, all three
 * outputs NULL.  n == 0 returns 0 without launching (*n_unique = 0).
 * rt_unique_scratch (-1 for a bad n) and rt_unique_geometry (the compiled-in
 * constants; any pointer may be NULL) are host arithmetic only. */
int rt_unique_count(uintptr_t stream, const void *keys, int64_t n, int dtype,
                    void *scratch, int64_t scratch_bytes, int64_t *n_unique);
int rt_unique_write(uintptr_t stream, const void *keys, const void *pos,
                    int64_t n, int dtype, void *scratch, void *out_keys,
                    void *out_first, void *out_counts);
int64_t rt_unique_scratch(int64_t n);
int rt_unique_geometry(int *block, int *keys_per_lane, int *grid_cap);

/* searchsorted — numpy.searchsorted (the reference has none).  v: m keys of
 * `dtype` (any rt_dtype), dense, sorted in the canonical order of
 * ramba_sortkey.h (raw bits; the caller's promise, as NumPy's).  Needles: a
 * strided box of 1..4 axes at `x + x_off`, same dtype, addressed as rt_hist
 * addresses its input (offset and strides in elements, any sign, zero
 * allowed).  out: dense C-order int64 over the box.  side 0 (left): the
 * number of keys that sort strictly before the needle; side 1 (right): the
 * number that do not sort after it.  Both in the canonical order: a NaN
 * needle lands at the first NaN (left) or after the last (right), and -0.0
 * and +0.0 are equal, as in NumPy.
 * Every search runs a FIXED number of branch-free trips (set on the host
 * from the sizes alone), so a wave does not diverge.  Two regimes by m:
 *   LDS    m <= lds_max[key width]: every block stages all of v, as
 *          canonical keys, in at most 64 KB of LDS (two blocks a CU) and
 *          grid-strides over the needles; no probe leaves the CU.
 *   FENCE  larger m: seg = ceil(m / fence); the block stages the keys v[0],
 *          v[seg], v[2 seg], .. (at most `fence`, a power of two; real keys
 *          only).  A needle searches the fence in LDS, log2(fence) trips,
 *          and finishes in one segment of at most seg keys in global memory.
 *          Exact for both sides and for duplicates that span fence entries
 *          (the argument is in DESIGN.md section 4g).
 * Needles take 16-byte loads under the rt_arg_flat_regime rule, else element
 * loads; at most grid_cap blocks of `block` lanes run.
 * Validated before any HIP call: nd, NULL shape / strides, extents, dtype,
 * side, m < 0 or >= 2^40, NULL v with m > 0, NULL x / out with work to do.
 * A zero extent returns 0 without launching; m == 0 writes zeros.
 * rt_searchsorted_geometry: the compiled-in constants (lds_max: 4 values,
 * for key widths 1, 2, 4 and 8 bytes; any pointer may be NULL); host
 * arithmetic only. */
int rt_searchsorted(uintptr_t stream, const void *v, int64_t m, const void *x,
                    int64_t x_off, int nd, const int64_t *shape,
                    const int64_t *strides, int dtype, int side, void *out);
int rt_searchsorted_geometry(int *block, int *fence, int64_t *lds_max,
                             int *grid_cap);

/* partition / argpartition — numpy.partition / numpy.argpartition (the
 * reference has neither): one stable split of a dense run about keys that
 * rt_select_pass found.  in: n raw keys of `dtype` (any rt_dtype).  pivots: a
 * HOST array of npiv, 1 <= npiv <= npiv_max (8), distinct ascending canonical
 * keys (ramba_sortkey.h), no bit set above the key width.  The bucket of a
 * key k is
 *     b(k) = 2 * (number of pivots < canon(k)) + (canon(k) equals a pivot),
 * 2 npiv + 1 buckets.  The output is the buckets in ascending order, each in
 * input order (a stable split); the raw bits are moved, so zero signs and NaN
 * payloads arrive as they were.  out (raw keys) or vals_out (int64 payloads)
 * may be NULL, not both; the payload of key i is vals_in[i], or val0 + i when
 * vals_in is NULL (vals_in = NULL, val0 = 0 is argpartition), as in rt_sort.
 * bucket_counts: HOST int64[2 npiv + 1], may be NULL; it receives the bucket
 * sizes.  When it is given the call synchronises the stream once, otherwise
 * not at all.
 * Three launches, none of which waits for another block, no atomics: the
 * output is the same from run to run.  (1) At most grid_cap blocks, each over
 * a contiguous range of tiles of block x keys_per_lane keys; a lane owns
 * keys_per_lane CONSECUTIVE keys, read with 16-byte loads when the run is
 * 16-byte aligned and the tile whole (else by element), computes their
 * buckets in registers (the pivots are kernel arguments) and counts them in
 * packed 16-bit fields, one per bucket but the last, whose counts are what is
 * left; one int64 per bucket and block goes to the scratch.  (2) One block
 * scans buckets and blocks.  (3) The same walk recomputes the buckets; a key
 * goes to its bucket's base for the block (advanced tile by tile) + the
 * counts of the waves below (a 4-entry LDS table) + one shuffle scan of the
 * packed words over the wave (every bucket's prefix at once) + the lane's
 * earlier keys, with direct stores.  npiv == 1, the top-k case, packs "below"
 * and "equal" into one 32-bit word and derives the third bucket; npiv <= 4
 * takes two 64-bit words, npiv <= 8 four.
 * `in` / vals_in are only read and must not overlap out, vals_out or the
 * scratch.  scratch: device memory, 16-byte aligned, of at least
 * rt_partition_scratch(n, npiv) bytes (two int64 per bucket and block, under
 * 1 MB).
 * Validated before any HIP call: dtype, n < 0 or >= 2^40, npiv, NULL /
 * unsorted / duplicate pivots, a pivot with bits above the key width, NULL in
 * / scratch with work to do, out and vals_out both NULL, a misaligned or too
 * small scratch.  n == 0 returns 0 without launching (bucket_counts zeroed).
 * rt_partition_scratch (-1 for a bad n or npiv) and rt_partition_geometry
 * (the compiled-in constants; any pointer may be NULL) are host arithmetic
 * only. */
int rt_partition(uintptr_t stream, const void *in, void *out,
                 const void *vals_in, int64_t val0, void *vals_out, int64_t n,
                 int dtype, int npiv, const uint64_t *pivots, void *scratch,
                 int64_t scratch_bytes, int64_t *bucket_counts);
int64_t rt_partition_scratch(int64_t n, int npiv);
int rt_partition_geometry(int *block, int *keys_per_lane, int *grid_cap,
                          int *npiv_max);

/* groupby reductions — the reference's ndarray.groupby(dim, labels,
 * num_groups).sum() / prod() / min() / max() / nanmean() (ramba.py:10290).
 * rt_group_reduce reads a strided box of 1..4 axes at `in + in_off` (offset
 * and strides in elements, any sign, zero allowed; dtype: any rt_dtype) whose
 * axis `axis` carries one group label per row, given as a CSR on the device:
 *   members  int32[shape[axis]]: the row numbers, stably sorted by label;
 *   seg      int32[ngroups + 1]: group g owns members[seg[g] .. seg[g + 1]).
 * out[.., g, ..] (extent ngroups on `axis`, out_strides in elements) receives
 * the reduction of group g's rows, the identity for an empty group.
 *   op       0 SUM, 1 PROD, 2 MIN, 3 MAX, 4 COUNT_VALID (the number of
 *            non-NaN members).
 *   out      SUM / PROD: the input's type for floats, int64 with wrap-around
 *            for integers; MIN / MAX: the input's type (RT_U8 is bool:
 *            identities 1 and 0); COUNT_VALID: int64.
 *   skipna   a NaN counts as the identity.  Without it NaN propagates; float
 *            MIN / MAX keep the first of two equal values.
 * No atomics: the order in which a group's members are combined is fixed by
 * the shape, the labels and the compiled-in constants, so the result is the
 * same from run to run.  Regimes (rt_group_regime; see ramba_rt.cpp):
 *   0 ROWS         another axis has the unit stride: lanes along it, a block
 *                  per (group, tile), members staged through LDS member_tile
 *                  at a time and combined in ascending order (a float SUM
 *                  equals the sequential np.add.at bit for bit); 16-byte
 *                  loads under the rule of rt_arg_flat_regime.
 *   1 ROWS_SPLIT   ROWS with fewer than split_blocks (group, 256 outputs)
 *                  pairs and shape[axis] >= 2 chunk + 1: member lists cut
 *                  into chunks of `chunk` rows, partials combined in order by
 *                  a second launch.
 *   2 LINE_SELECT  the group axis has the unit stride, ngroups <= select_max:
 *                  select_max compare-select register accumulators per lane,
 *                  a shuffle tree, LDS, per-block partials combined in order.
 *   3 LINE_GATHER  the same with more groups: a wave per (line, chunk of
 *                  gather_chunk members), a shuffle tree, chunks in order.
 * scratch: device memory, 16-byte aligned, of at least rt_group_scratch(..)
 * bytes (0 in regime ROWS; NULL is then accepted).  in / members / seg are
 * only read and must not overlap out or the scratch.
 * Validated before any HIP call: nd, NULL shape / strides / out_strides,
 * extents, axis, dtype, op, ngroups < 1 or >= 2^31, shape[axis] >= 2^31, a
 * result beyond 2^46 elements, NULL in / members / seg / out / scratch with
 * work to do, a misaligned scratch.  A zero extent returns 0 without
 * launching.  rt_group_regime (-1 for bad arguments), rt_group_scratch (-1
 * likewise) and rt_group_geometry (the compiled-in constants; any pointer may
 * be NULL) are host arithmetic only. */
int rt_group_reduce(uintptr_t stream, const void *in, int64_t in_off, int nd,
                    const int64_t *shape, const int64_t *strides, int axis,
                    int dtype, int op, int skipna, const void *members,
                    const void *seg, int64_t ngroups, void *out,
                    const int64_t *out_strides, void *scratch);
int64_t rt_group_scratch(int nd, const int64_t *shape, const int64_t *strides,
                         int axis, int dtype, int op, int64_t ngroups);
int rt_group_regime(int nd, const int64_t *shape, const int64_t *strides,
                    int axis, int dtype, int64_t ngroups);
int rt_group_geometry(int *block, int *member_tile, int *chunk,
                      int *split_blocks, int *select_max, int *select_blocks,
                      int *gather_chunk, int *grid_cap);

int rt_stream_sync(uintptr_t stream);
int rt_device_sync(void);

/* HIP-event timing for the bench's roofline leg. */
int   rt_event_create(void **ev);
int   rt_event_destroy(void *ev);
int   rt_event_record(void *ev, uintptr_t stream);
/* elapsed ms between two recorded events (synchronises on `end`) */
int   rt_event_elapsed(void *start, void *end, float *ms);

#ifdef __cplusplus
}
#endif

#endif /* RAMBA_RT_H */
