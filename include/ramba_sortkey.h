/* ramba_sortkey — the order of sort / argsort and of the order statistics.
 *
 * ONE function decides every digit and every comparison: the radix passes of
 * rt_sort, the compare-exchanges of rt_sort_lines and the binary search of
 * rt_sort_bounds all read rt_sort_canon(raw bits), an unsigned key of the
 * element's width whose unsigned order is NumPy's sort order:
 *
 *   - integers: numeric order (the sign bit is flipped); RT_U8 (bool and
 *     uint8) is its own key;
 *   - floats: -inf < ... < -0.0 == +0.0 < ... < +inf < NaN.  The usual
 *     sign-dependent flip (negative: all bits; else: the sign bit), after
 *     -0.0 has been given the bits of +0.0 and any NaN, of either sign and
 *     any payload, has become all ones.  No number maps to all ones: the
 *     bit pattern that would is itself a NaN;
 *   - ties, equal keys, are broken by ascending position in the sorted run,
 *     which makes the order total and the result that of
 *     numpy.sort(kind="stable") / numpy.argsort(kind="stable") bit for bit.
 *
 * The kernels MOVE THE RAW BITS and take digits and comparisons from the
 * canonical key on the fly, so the sign of every zero and the payload of
 * every NaN arrive as they were.  Padding of a short line is the pair (all
 * ones, a position past the line), which sorts after every real element,
 * NaN included.
 *
 * Plain C++: tests may compile this header for the host.
 */

#ifndef RAMBA_SORTKEY_H
#define RAMBA_SORTKEY_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_SORT_HD __host__ __device__ __forceinline__
#else
#define RT_SORT_HD inline
#endif

/* rt_sort_key<T>::U is the unsigned type of T's width, FLT says whether the
 * bits are an IEEE float. */
template <typename T> struct rt_sort_key;
template <> struct rt_sort_key<double>  { typedef uint64_t U; enum { FLT = 1, SGN = 1 }; };
template <> struct rt_sort_key<float>   { typedef uint32_t U; enum { FLT = 1, SGN = 1 }; };
template <> struct rt_sort_key<int64_t> { typedef uint64_t U; enum { FLT = 0, SGN = 1 }; };
template <> struct rt_sort_key<int32_t> { typedef uint32_t U; enum { FLT = 0, SGN = 1 }; };
template <> struct rt_sort_key<int16_t> { typedef uint16_t U; enum { FLT = 0, SGN = 1 }; };
template <> struct rt_sort_key<int8_t>  { typedef uint8_t U;  enum { FLT = 0, SGN = 1 }; };
template <> struct rt_sort_key<uint8_t> { typedef uint8_t U;  enum { FLT = 0, SGN = 0 }; };

/* the canonical key of the raw bits `u` of an element of type T */
template <typename T>
RT_SORT_HD typename rt_sort_key<T>::U
rt_sort_canon(typename rt_sort_key<T>::U u) {
    typedef typename rt_sort_key<T>::U U;
    const U sign = (U)((U)1 << (8 * sizeof(U) - 1));
    if (rt_sort_key<T>::FLT) {
        /* exponent mask: 8 bits below the sign for float, 11 for double */
        const int mbits = sizeof(U) == 4 ? 23 : 52;
        const U inf = (U)((U)(sign - 1) >> mbits << mbits);
        const U mag = (U)(u & (U)(sign - 1));
        if (mag > inf) return (U)~(U)0;          /* NaN */
        if (mag == 0) return sign;               /* +0.0 and -0.0 */
        return (u & sign) ? (U)~u : (U)(u | sign);
    }
    return rt_sort_key<T>::SGN ? (U)(u ^ sign) : u;
}

/* The inverse: the raw bits of the element that a canonical key stands for.
 * Exact for integers and for every float but the two the key does not tell
 * apart: a zero comes back as +0.0 and a NaN as the one quiet NaN with a
 * clear sign and an empty payload.  rt_sort_canon(rt_sort_decode(k)) == k for
 * every key that rt_sort_canon can return.  Selection (rt_select_pass) finds
 * an order statistic as a key and decodes it here, so no raw element is ever
 * carried. */
template <typename T>
RT_SORT_HD typename rt_sort_key<T>::U
rt_sort_decode(typename rt_sort_key<T>::U k) {
    typedef typename rt_sort_key<T>::U U;
    const U sign = (U)((U)1 << (8 * sizeof(U) - 1));
    if (rt_sort_key<T>::FLT) {
        const int mbits = sizeof(U) == 4 ? 23 : 52;
        if (k == (U)~(U)0)                      /* NaN: exponent | quiet bit */
            return (U)((U)(sign - 1) >> (mbits - 1) << (mbits - 1));
        return (k & sign) ? (U)(k ^ sign) : (U)~k;
    }
    return rt_sort_key<T>::SGN ? (U)(k ^ sign) : k;
}

#endif /* RAMBA_SORTKEY_H */
