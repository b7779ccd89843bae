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
 * rt_mask_compact, rt_axis_scan and rt_flat_copy (the contract of
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
