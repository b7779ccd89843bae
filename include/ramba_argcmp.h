/* ramba_argcmp — the (value, index) pair order of argmax / argmin /
 * nanargmax / nanargmin.
 *
 * ONE function decides every merge: the per-thread accumulate, the wave
 * shuffles, the LDS tree, the per-block and per-chunk second stages, the
 * cross-rank pair combine (rt_arg_combine_box) and, restated in NumPy, the
 * host merge of runtime.arg_reduce_op.  Indices are GLOBAL (the coordinate
 * along the reduced axis, or the C-order flat position in the view), so the
 * order is total and a merge gives the same pair whatever the grouping:
 * results are deterministic without atomics.
 *
 *   - idx < 0 means "nothing here" and always loses;
 *   - unless skipna, a NaN beats every number and the lowest-index NaN
 *     beats the other NaNs (NumPy: the first NaN wins);
 *   - with skipna a NaN never wins (callers also drop NaNs at load, giving
 *     an all-NaN line idx -1);
 *   - otherwise > for max and < for min, and on equal values (0.0 == -0.0)
 *     the lower index.
 *
 * Integer instantiations compare as integers (v != v folds to false); no
 * value is routed through a double.  Plain C++: tests compile this header
 * for the host.
 */

#ifndef RAMBA_ARGCMP_H
#define RAMBA_ARGCMP_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_ARG_HD __host__ __device__ __forceinline__
#else
#define RT_ARG_HD inline
#endif

/* true when pair p = (pv, pi) replaces pair q = (qv, qi).
 *
 * LATER = true is the caller's promise that p is a real element (pi >= 0)
 * whose index is above q's: a thread walking its elements in increasing
 * index order.  p then wins only by being strictly better, pi is not read,
 * and with constant is_max / skipna the test folds to a few instructions. */
template <typename T, bool LATER = false>
RT_ARG_HD bool rt_arg_better(T pv, int64_t pi, T qv, int64_t qi, int is_max,
                             int skipna) {
    if (!LATER && pi < 0) return false;
    const bool pn = pv != pv, qn = qv != qv;
    if (skipna) {
        if (pn) return false;
        if (qi < 0 || qn) return true;
    } else {
        if (qi < 0) return true;
        if (pn || qn) return pn && (!qn || (!LATER && pi < qi));
    }
    if (is_max ? pv > qv : pv < qv) return true;
    return !LATER && pv == qv && pi < qi;
}

#endif /* RAMBA_ARGCMP_H */
