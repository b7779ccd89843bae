// ramba_rt — C-ABI runtime: hiprtc JIT cache, kernel launcher, strided box
// copies.  See include/ramba_rt.h for the boundary contract and the
// reference interfaces each entry point replaces.
//
// Build (in-tree, build() in __graft_entry__.py):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared \
//       ramba_amd/csrc/ramba_rt.cpp -o ramba_amd/_lib/libramba_rt.so -lhiprtc

#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/ramba_rt.h"

namespace {

std::mutex g_mutex;
std::string g_last_error;

void set_error(const std::string &msg) {
    std::lock_guard<std::mutex> lk(g_mutex);
    g_last_error = msg;
}

#define HIP_CHECK(expr)                                                    \
    do {                                                                   \
        hipError_t _e = (expr);                                            \
        if (_e != hipSuccess) {                                            \
            set_error(std::string(#expr) + ": " + hipGetErrorString(_e));  \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int fail(const char *who, const char *what) {
    set_error(std::string(who) + ": " + what);
    return 1;
}

// Host-side geometry check shared by the box-shaped entry points
// (rt_copy_box, rt_combine_box, rt_mask_compact, rt_axis_scan,
// rt_flat_copy); runs before any HIP call.  Extents may be zero (the entry
// then returns 0 without launching) but not negative; the size limits are
// those of rt_arg_* (an extent under 2^40, a product of at most 2^46), so
// no element count or flat index can overflow int64.  *n_out = product.
int box_extents(const char *who, int nd, int nd_min, const int64_t *shape,
                const int64_t *str_a, const int64_t *str_b, int64_t *n_out) {
    if (nd < nd_min || nd > 4) return fail(who, "nd out of range");
    if (!shape) return fail(who, "NULL shape");
    if (!str_a || !str_b) return fail(who, "NULL strides");
    int64_t n = 1;
    bool empty = false;
    for (int d = 0; d < nd; ++d) {
        if (shape[d] < 0) return fail(who, "negative extent in shape");
        if (shape[d] >= (1LL << 40))
            return fail(who, "extent in shape out of range");
        if (shape[d] == 0) empty = true;
    }
    for (int d = 0; d < nd && !empty; ++d) {
        if (n > (1LL << 46) / shape[d])
            return fail(who, "shape too large (extent product overflows)");
        n *= shape[d];
    }
    *n_out = empty ? 0 : n;
    return 0;
}

// Status of the kernel launch(es) just issued; a failure is reported as
// "<what> launch: <hip error>".
int launched(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error(std::string(what) + " launch: " + hipGetErrorString(e));
        return 1;
    }
    return 0;
}

// The one rt_dtype -> element type mapping: runs call(T()) for the type of
// `dtype`.  NCODES is how many codes the entry point accepts, 4 (RT_F64 ..
// RT_I32) or 7 (all); the types of the other codes are never instantiated.
// Entry points range-check dtype with their other arguments, so the last
// line is not reached from them.
template <int NCODES, typename F>
int dtype_dispatch(const char *who, int dtype, F call) {
    static_assert(NCODES == 4 || NCODES == 7, "4 or 7 dtype codes");
    switch (dtype) {
        case RT_F64: return call(double());
        case RT_F32: return call(float());
        case RT_I64: return call(int64_t());
        case RT_I32: return call(int32_t());
    }
    if constexpr (NCODES == 7) {
        switch (dtype) {
            case RT_I16: return call(int16_t());
            case RT_I8: return call(int8_t());
            case RT_U8: return call(uint8_t());
        }
    }
    return fail(who, "bad dtype");
}

// element size of a (range-checked) rt_dtype code
int dtype_size(int dtype) {
    return dtype_dispatch<7>("dtype_size", dtype,
                             [](auto t) { return (int)sizeof(t); });
}

// Kernel geometry: copy nd extents and one or two stride lists into the
// 4-slot arrays of an argument struct, padding the unused axes with extent
// 1, stride 0.
void fill_geom(int nd, const int64_t *shape, int64_t *gshape,
               const int64_t *str_a, int64_t *gstr_a,
               const int64_t *str_b = nullptr, int64_t *gstr_b = nullptr) {
    for (int d = 0; d < 4; ++d) {
        gshape[d] = d < nd ? shape[d] : 1;
        gstr_a[d] = d < nd ? str_a[d] : 0;
        if (gstr_b) gstr_b[d] = d < nd ? str_b[d] : 0;
    }
}

struct Kernel {
    hipModule_t module = nullptr;
    hipFunction_t func = nullptr;
};

std::unordered_map<std::string, Kernel *> g_kernels;

// content-addressed on-disk cache of compiled code objects (RAMBA_KCACHE):
// filenames are a 128-bit FNV hash of the SOURCE, so stale entries are
// impossible; pre-populated by the CPU test suite (hiprtc needs no GPU)
// and shipped with the repo snapshot.
std::string kcache_path(const char *source) {
    const char *dir = getenv("RAMBA_KCACHE");
    if (!dir || !*dir) return "";
    uint64_t h1 = 1469598103934665603ull, h2 = 14695981039346656037ull;
    for (const char *p = source; *p; ++p) {
        h1 = (h1 ^ (unsigned char)*p) * 1099511628211ull;
        h2 = (h2 * 1099511628211ull) ^ (unsigned char)*p;
    }
    char buf[64];
    snprintf(buf, sizeof(buf), "/%016llx%016llx.hsaco",
             (unsigned long long)h1, (unsigned long long)h2);
    return std::string(dir) + buf;
}

bool kcache_read(const std::string &path, std::vector<char> &out) {
    if (path.empty()) return false;
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) return false;
    std::streamsize sz = f.tellg();
    if (sz <= 0) return false;
    out.resize(sz);
    f.seekg(0);
    return bool(f.read(out.data(), sz));
}

void kcache_write(const std::string &path, const std::vector<char> &code) {
    if (path.empty()) return;
    std::string tmp = path + ".tmp";
    std::ofstream f(tmp, std::ios::binary);
    if (!f) return;
    f.write(code.data(), code.size());
    f.close();
    rename(tmp.c_str(), path.c_str());
}

int compile_to_code(const char *source, std::vector<char> &code) {
    hiprtcProgram prog;
    hiprtcResult r =
        hiprtcCreateProgram(&prog, source, "fused.hip", 0, nullptr, nullptr);
    if (r != HIPRTC_SUCCESS) {
        set_error(std::string("hiprtcCreateProgram: ") +
                  hiprtcGetErrorString(r));
        return 1;
    }
    const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17",
                          "-ffp-contract=off"};
    r = hiprtcCompileProgram(prog, 4, opts);
    if (r != HIPRTC_SUCCESS) {
        size_t logsz = 0;
        hiprtcGetProgramLogSize(prog, &logsz);
        std::string log(logsz, '\0');
        if (logsz) hiprtcGetProgramLog(prog, log.data());
        hiprtcDestroyProgram(&prog);
        set_error("hiprtc compile failed:\n" + log);
        return 1;
    }
    size_t codesz = 0;
    hiprtcGetCodeSize(prog, &codesz);
    code.resize(codesz);
    hiprtcGetCode(prog, code.data());
    hiprtcDestroyProgram(&prog);
    return 0;
}

}  // namespace

extern "C" {

const char *rt_last_error(void) { return g_last_error.c_str(); }

int rt_init(int device) {
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipFree(nullptr));  // force context creation
    return 0;
}

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// Compile-only check (no module load — works without a GPU).  Used by the
// CPU test suite to validate generated source against hiprtc/gfx950.
int rt_compile_check(const char *source) {
    std::string path = kcache_path(source);
    std::vector<char> code;
    if (kcache_read(path, code)) return 0;   // already compiled
    if (compile_to_code(source, code)) return 1;
    kcache_write(path, code);
    return 0;
}

int rt_kernel_get(const char *key, const char *source, const char *kname,
                  void **out_kernel) {
    {
        std::lock_guard<std::mutex> lk(g_mutex);
        auto it = g_kernels.find(key);
        if (it != g_kernels.end()) {
            *out_kernel = it->second;
            return 0;
        }
    }
    std::string path = kcache_path(source);
    std::vector<char> code;
    if (!kcache_read(path, code)) {
        if (compile_to_code(source, code)) return 1;
        kcache_write(path, code);
    }

    Kernel *k = new Kernel();
    hipError_t e = hipModuleLoadData(&k->module, code.data());
    if (e != hipSuccess) {
        set_error(std::string("hipModuleLoadData: ") + hipGetErrorString(e));
        delete k;
        return 1;
    }
    e = hipModuleGetFunction(&k->func, k->module, kname);
    if (e != hipSuccess) {
        set_error(std::string("hipModuleGetFunction(") + kname +
                  "): " + hipGetErrorString(e));
        delete k;
        return 1;
    }
    {
        std::lock_guard<std::mutex> lk(g_mutex);
        g_kernels[key] = k;
    }
    *out_kernel = k;
    return 0;
}

int rt_launch(void *kernel, unsigned gx, unsigned gy, unsigned gz,
              unsigned bx, uintptr_t stream, const void *args,
              size_t argsize) {
    Kernel *k = static_cast<Kernel *>(kernel);
    size_t sz = argsize;
    void *config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, const_cast<void *>(args),
                      HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz,
                      HIP_LAUNCH_PARAM_END};
    HIP_CHECK(hipModuleLaunchKernel(k->func, gx, gy, gz, bx, 1, 1, 0,
                                    reinterpret_cast<hipStream_t>(stream),
                                    nullptr, config));
    return 0;
}

int rt_stream_sync(uintptr_t stream) {
    HIP_CHECK(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    return 0;
}

int rt_device_sync(void) {
    HIP_CHECK(hipDeviceSynchronize());
    return 0;
}

int rt_event_create(void **ev) {
    hipEvent_t e;
    HIP_CHECK(hipEventCreate(&e));
    *ev = e;
    return 0;
}

int rt_event_destroy(void *ev) {
    HIP_CHECK(hipEventDestroy(static_cast<hipEvent_t>(ev)));
    return 0;
}

int rt_event_record(void *ev, uintptr_t stream) {
    HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(ev),
                             reinterpret_cast<hipStream_t>(stream)));
    return 0;
}

int rt_event_elapsed(void *start, void *end, float *ms) {
    HIP_CHECK(hipEventSynchronize(static_cast<hipEvent_t>(end)));
    HIP_CHECK(hipEventElapsedTime(ms, static_cast<hipEvent_t>(start),
                                  static_cast<hipEvent_t>(end)));
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// strided box copy kernels (pack / unpack / halo / gather)
// One thread per element; multi-index from a flattened id (boxes are small:
// halo slabs, message buffers).  nd <= 4, shapes/strides in elements.
// ---------------------------------------------------------------------------

namespace {

struct BoxArgs {
    int64_t n;                // total elements
    int64_t shape[4];
    int64_t dstr[4];
    int64_t sstr[4];
    int nd;
};

template <typename T>
__global__ __launch_bounds__(256) void box_copy_kernel(T *__restrict__ dst,
                                                       const T *__restrict__ src,
                                                       BoxArgs a) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < a.n; i += stride) {
        int64_t rem = i, so = 0, dofs = 0;
        for (int d = a.nd - 1; d >= 0; --d) {
            int64_t idx = rem % a.shape[d];
            rem /= a.shape[d];
            so += idx * a.sstr[d];
            dofs += idx * a.dstr[d];
        }
        dst[dofs] = src[so];
    }
}

template <typename T>
int box_copy_launch(uintptr_t stream, void *dst, const void *src,
                    const BoxArgs &a) {
    int64_t blocks = (a.n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(box_copy_kernel<T>, dim3((unsigned)blocks), dim3(256),
                       0, reinterpret_cast<hipStream_t>(stream),
                       static_cast<T *>(dst), static_cast<const T *>(src), a);
    return launched("box_copy");
}

}  // namespace

// ---------------------------------------------------------------------------
// typed combining box copy: dst = dst OP src  (axis-reduction cross-rank
// merge — replaces the reference's internal_reduction2 slice-combining,
// ramba/ramba.py:5818-5849)
// ---------------------------------------------------------------------------

namespace {

template <typename T, int OP>
__global__ __launch_bounds__(256) void box_combine_kernel(
    T *__restrict__ dst, const T *__restrict__ src, BoxArgs a) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < a.n; i += stride) {
        int64_t rem = i, so = 0, dofs = 0;
        for (int d = a.nd - 1; d >= 0; --d) {
            int64_t idx = rem % a.shape[d];
            rem /= a.shape[d];
            so += idx * a.sstr[d];
            dofs += idx * a.dstr[d];
        }
        T s = src[so], d0 = dst[dofs];
        if (OP == 0) dst[dofs] = d0 + s;
        else if (OP == 1) dst[dofs] = d0 * s;
        // NaN-propagating min/max (NumPy semantics): a NaN in s loses
        // every comparison, so take it explicitly; a NaN in d0 stays.
        // s != s is constant-false for the integer instantiations.
        else if (OP == 2) dst[dofs] = (s < d0 || s != s) ? s : d0;
        else if (OP == 3) dst[dofs] = (s > d0 || s != s) ? s : d0;
        else if (OP == 4) dst[dofs] = (d0 != (T)0 && s != (T)0) ? (T)1 : (T)0;
        else dst[dofs] = (d0 != (T)0 || s != (T)0) ? (T)1 : (T)0;
    }
}

template <typename T>
int box_combine_launch(uintptr_t stream, void *dst, const void *src,
                       const BoxArgs &a, int op) {
    int64_t blocks = (a.n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    T *d = static_cast<T *>(dst);
    const T *s = static_cast<const T *>(src);
    switch (op) {
#define CASE(n)                                                            \
    case n:                                                                \
        hipLaunchKernelGGL((box_combine_kernel<T, n>), dim3((unsigned)blocks), \
                           dim3(256), 0, st, d, s, a);                     \
        break;
        CASE(0) CASE(1) CASE(2) CASE(3) CASE(4) CASE(5)
#undef CASE
        default:
            set_error("rt_combine_box: bad op");
            return 1;
    }
    return launched("box_combine");
}

}  // namespace

// dtype: any rt_dtype; op: 0=add 1=mul 2=min 3=max 4=logical_and
// 5=logical_or
extern "C" int rt_combine_box(uintptr_t stream, void *dst, const void *src,
                              int nd, const int64_t *shape,
                              const int64_t *dst_strides,
                              const int64_t *src_strides, int64_t dst_off,
                              int64_t src_off, int dtype, int op) {
    BoxArgs a;
    if (box_extents("rt_combine_box", nd, 1, shape, dst_strides, src_strides,
                    &a.n))
        return 1;
    if (dtype < RT_F64 || dtype > RT_U8)
        return fail("rt_combine_box", "bad dtype");
    if (op < 0 || op > 5) return fail("rt_combine_box", "bad op");
    if (a.n == 0) return 0;
    if (!dst || !src) return fail("rt_combine_box", "NULL dst/src");
    a.nd = nd;
    fill_geom(nd, shape, a.shape, dst_strides, a.dstr, src_strides, a.sstr);
    return dtype_dispatch<7>("rt_combine_box", dtype, [&](auto t) {
        using T = decltype(t);
        return box_combine_launch<T>(stream, static_cast<T *>(dst) + dst_off,
                                     static_cast<const T *>(src) + src_off,
                                     a, op);
    });
}

extern "C" int rt_copy_box(uintptr_t stream, void *dst, const void *src,
                           int nd, const int64_t *shape,
                           const int64_t *dst_strides,
                           const int64_t *src_strides, int64_t dst_off,
                           int64_t src_off, int elemsize) {
    BoxArgs a;
    if (box_extents("rt_copy_box", nd, 1, shape, dst_strides, src_strides,
                    &a.n))
        return 1;
    if (elemsize != 1 && elemsize != 2 && elemsize != 4 && elemsize != 8)
        return fail("rt_copy_box", "bad elemsize");
    if (a.n == 0) return 0;
    if (!dst || !src) return fail("rt_copy_box", "NULL dst/src");
    a.nd = nd;
    fill_geom(nd, shape, a.shape, dst_strides, a.dstr, src_strides, a.sstr);
    char *d8 = static_cast<char *>(dst) + dst_off * elemsize;
    const char *s8 = static_cast<const char *>(src) + src_off * elemsize;
    switch (elemsize) {
        case 1: return box_copy_launch<uint8_t>(stream, d8, s8, a);
        case 2: return box_copy_launch<uint16_t>(stream, d8, s8, a);
        case 4: return box_copy_launch<uint32_t>(stream, d8, s8, a);
        case 8: return box_copy_launch<uint64_t>(stream, d8, s8, a);
        default:
            set_error("rt_copy_box: bad elemsize");
            return 1;
    }
}

// ---------------------------------------------------------------------------
// cumsum (replaces the reference's scumulative local-prefix +
// cross-worker fixup chain, ramba/ramba.py:10057-10171 / 3378-3460):
// three-phase local scan (block sums -> block-sum scan + total -> apply),
// the cross-rank offset comes from an allgather in the host runtime.
// ---------------------------------------------------------------------------

namespace {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 16;
constexpr int SCAN_CHUNK = SCAN_THREADS * SCAN_ITEMS;

// LDS index of chunk element g in the staged kernels (cumsum_k3,
// mask_write_k): one pad element per 16 keeps a thread's contiguous reads
// off a 32-way bank conflict
#define LIDX(g) ((g) + ((g) >> 4))

template <typename T>
__global__ __launch_bounds__(256) void cumsum_k1(const T *__restrict__ in,
                                                 int64_t in_off,
                                                 int64_t in_stride, int64_t n,
                                                 T *__restrict__ bsums) {
    int64_t blk = blockIdx.x;
    int64_t nblocks = gridDim.x;
    for (; blk * SCAN_CHUNK < n; blk += nblocks) {
        int64_t base = blk * SCAN_CHUNK;
        T acc = (T)0;
        for (int j = 0; j < SCAN_ITEMS; ++j) {
            int64_t i = base + j * SCAN_THREADS + threadIdx.x;
            if (i < n) acc += in[in_off + i * in_stride];
        }
        // wave + LDS tree sum
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        __shared__ T lds[4];
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0)
            bsums[blk] = lds[0] + lds[1] + lds[2] + lds[3];
        __syncthreads();
    }
}

// one block: in-place EXCLUSIVE scan of bsums; writes the grand total
template <typename T>
__global__ __launch_bounds__(256) void cumsum_k2(T *__restrict__ bsums,
                                                 int64_t nblocks,
                                                 T *__restrict__ total) {
    // each thread owns a contiguous range of block sums
    int64_t per = (nblocks + SCAN_THREADS - 1) / SCAN_THREADS;
    int64_t lo = threadIdx.x * per;
    int64_t hi = lo + per < nblocks ? lo + per : nblocks;
    T s = (T)0;
    for (int64_t i = lo; i < hi; ++i) s += bsums[i];
    // exclusive scan of the 256 per-thread sums (wave shfl_up + LDS)
    T x = s;
    int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        T y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    __shared__ T wsum[4];
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    T wbase = (T)0;
    for (int w = 0; w < wid; ++w) wbase += wsum[w];
    // exclusive prefix of this thread's range: the lane below's inclusive
    // value, NOT x - s (a NaN or inf in s would poison the prefix of the
    // elements BEFORE it: inf - inf and nan - nan are nan)
    T below = __shfl_up(x, 1, 64);
    T excl = wbase + (lane > 0 ? below : (T)0);
    // rewrite this thread's range as exclusive prefixes
    T run = excl;
    for (int64_t i = lo; i < hi; ++i) {
        T v = bsums[i];
        bsums[i] = run;
        run += v;
    }
    // thread 255's final `run` is the grand total (its range is the last
    // non-empty one, or empty with excl == sum of everything before)
    if (threadIdx.x == SCAN_THREADS - 1 && total) *total = run;
}

template <typename T>
__global__ __launch_bounds__(256) void cumsum_k3(const T *__restrict__ in,
                                                 int64_t in_off,
                                                 int64_t in_stride, int64_t n,
                                                 T *__restrict__ out,
                                                 int64_t out_off,
                                                 const T *__restrict__ bsums,
                                                 T base) {
    // stage the chunk through LDS so global loads AND stores stay
    // coalesced (per-lane contiguous-16 global stores are partial-line
    // read-modify-write: measured 572 GB/s -> LDS-staged ~streaming
    // rate).  One pad element per 16 (LIDX) keeps the per-thread contiguous
    // reads off a 32-way bank conflict.  ~35 KB of LDS for fp64 chunks.
    __shared__ T lds[SCAN_CHUNK + SCAN_THREADS];
    int64_t blk = blockIdx.x;
    int64_t nblocks = gridDim.x;
    for (; blk * SCAN_CHUNK < n; blk += nblocks) {
        int64_t b0 = blk * SCAN_CHUNK;
        // coalesced load into LDS
        for (int j = 0; j < SCAN_ITEMS; ++j) {
            int64_t i = b0 + j * SCAN_THREADS + threadIdx.x;
            if (i < n) lds[LIDX(j * SCAN_THREADS + threadIdx.x)] =
                in[in_off + i * in_stride];
        }
        __syncthreads();
        // per-thread sum of its contiguous 16 LDS elements
        int64_t l0 = (int64_t)threadIdx.x * SCAN_ITEMS;
        int64_t lmax = n - b0;
        T s = (T)0;
        for (int j = 0; j < SCAN_ITEMS; ++j)
            if (l0 + j < lmax) s += lds[LIDX(l0 + j)];
        // exclusive scan across the block's threads
        T x = s;
        int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
        for (int off = 1; off < 64; off <<= 1) {
            T y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        __shared__ T wsum[4];
        if (lane == 63) wsum[wid] = x;
        __syncthreads();
        T wbase = (T)0;
        for (int w = 0; w < wid; ++w) wbase += wsum[w];
        // exclusive thread prefix from the lane below (x - s would turn a
        // NaN/inf in this thread's items into NaN for the items before it)
        T below = __shfl_up(x, 1, 64);
        T run = base + bsums[blk] + wbase + (lane > 0 ? below : (T)0);
        for (int j = 0; j < SCAN_ITEMS; ++j) {
            if (l0 + j < lmax) {
                run += lds[LIDX(l0 + j)];
                lds[LIDX(l0 + j)] = run;
            }
        }
        __syncthreads();
        // coalesced store from LDS
        for (int j = 0; j < SCAN_ITEMS; ++j) {
            int64_t i = b0 + j * SCAN_THREADS + threadIdx.x;
            if (i < n) out[out_off + i] =
                lds[LIDX(j * SCAN_THREADS + threadIdx.x)];
        }
        __syncthreads();
    }
}

template <typename T>
int cumsum_launch(uintptr_t stream, const void *in, int64_t in_off,
                  int64_t in_stride, int64_t n, void *out, int64_t out_off,
                  void *bsums, int64_t nblocks, void *total, double fbase,
                  int64_t ibase, int phase) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned grid = (unsigned)nblocks;
    if (phase == 1) {
        hipLaunchKernelGGL((cumsum_k1<T>), dim3(grid), dim3(SCAN_THREADS), 0,
                           st, static_cast<const T *>(in), in_off, in_stride,
                           n, static_cast<T *>(bsums));
    } else if (phase == 2) {
        hipLaunchKernelGGL((cumsum_k2<T>), dim3(1), dim3(SCAN_THREADS), 0, st,
                           static_cast<T *>(bsums), nblocks,
                           static_cast<T *>(total));
    } else if (phase == 3) {
        T base = (T)fbase;
        if (sizeof(T) >= 4 && (T)0.5 == 0) base = (T)ibase;  // integer T
        hipLaunchKernelGGL((cumsum_k3<T>), dim3(grid), dim3(SCAN_THREADS), 0,
                           st, static_cast<const T *>(in), in_off, in_stride,
                           n, static_cast<T *>(out), out_off,
                           static_cast<const T *>(bsums), base);
    } else {
        return fail("rt_cumsum", "bad phase");
    }
    return launched("cumsum");
}

}  // namespace

// dtype: RT_F64 .. RT_I32; phase 1/2/3 (see kernel comments)
extern "C" int rt_cumsum(uintptr_t stream, const void *in, int64_t in_off,
                         int64_t in_stride, int64_t n, void *out,
                         int64_t out_off, void *bsums, int64_t nblocks,
                         void *total, double fbase, int64_t ibase,
                         int dtype, int phase) {
    if (dtype < RT_F64 || dtype > RT_I32)
        return fail("rt_cumsum", "bad dtype");
    if (phase < 1 || phase > 3) return fail("rt_cumsum", "bad phase");
    if (n < 0) return fail("rt_cumsum", "negative n");
    // phases 1 and 3 use nblocks as their grid (the kernels stride over the
    // chunks of n); phase 2 scans bsums[0, nblocks) in one block
    if (nblocks < 1) return fail("rt_cumsum", "nblocks < 1");
    if (nblocks >= (1LL << 31)) return fail("rt_cumsum", "nblocks too large");
    if (phase != 2 && n == 0) return 0;
    if (!bsums) return fail("rt_cumsum", "NULL bsums");
    if (phase != 2 && !in) return fail("rt_cumsum", "NULL in");
    if (phase == 3 && !out) return fail("rt_cumsum", "NULL out");
    return dtype_dispatch<4>("rt_cumsum", dtype, [&](auto t) {
        return cumsum_launch<decltype(t)>(stream, in, in_off, in_stride, n,
                                          out, out_off, bsums, nblocks,
                                          total, fbase, ibase, phase);
    });
}

// ---------------------------------------------------------------------------
// ordered boolean-mask compaction (SURVEY §8f n3 second half; the
// reference's compressing boolean getitem `a[mask]`, ramba.py maskarray
// getitem path).  Three phases over the rank's local box, C iteration
// order: (1) per-chunk selected counts, (2) exclusive scan of the chunk
// counts (reuses rt_cumsum phase 2 with dtype i64), (3) ordered write of
// the selected elements into a dense output at chunk_base + intra-chunk
// exclusive prefix.  Cross-rank ordering is the host runtime's job
// (allgather of local counts -> uneven result divisions).
// ---------------------------------------------------------------------------

namespace {

constexpr int MC_ITEMS = 8;                  // 2048-elem chunks: ~34 KB
constexpr int MC_CHUNK = 256 * MC_ITEMS;     // LDS -> 4 blocks/CU

struct MCArgs {
    int64_t n;
    int64_t shape[4];
    int64_t astr[4];   // element strides of a over the box
    int64_t mstr[4];   // element strides of the mask over the box
    int nd;
};

__device__ __forceinline__ int64_t mc_addr(const MCArgs &g, int64_t i,
                                           const int64_t *str) {
    if (g.nd == 1) return i * str[0];   // int64 div costs ~100 cycles
    int64_t rem = i, off = 0;
    for (int d = g.nd - 1; d >= 0; --d) {
        int64_t idx = rem % g.shape[d];
        rem /= g.shape[d];
        off += idx * str[d];
    }
    return off;
}

// vectorised count for contiguous 1-D masks: one uint64 load per lane
// (the byte-granular version issued one VMEM op per byte; count pass was
// 0.85 TB/s).  The caller guarantees 8-B pointer alignment (core offsets
// are 128-B multiples by the pad design).
__global__ __launch_bounds__(256) void mask_count_vec_k(
    const uint8_t *__restrict__ m, int64_t n,
    int64_t *__restrict__ bcounts) {
    __shared__ int64_t lds[4];
    int64_t blk = blockIdx.x;
    int64_t nblocks = gridDim.x;
    const unsigned long long *m8 =
        reinterpret_cast<const unsigned long long *>(m);
    for (; blk * MC_CHUNK < n; blk += nblocks) {
        int64_t i0 = blk * MC_CHUNK + (int64_t)threadIdx.x * 8;
        int64_t acc = 0;
        if (i0 + 8 <= n) {
            unsigned long long v = m8[i0 >> 3];
            for (int b = 0; b < 8; ++b)
                acc += ((v >> (8 * b)) & 0xffULL) != 0;
        } else {
            for (int64_t i = i0; i < n && i < i0 + 8; ++i)
                acc += m[i] != 0;
        }
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0)
            bcounts[blk] = lds[0] + lds[1] + lds[2] + lds[3];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void mask_count_k(
    const uint8_t *__restrict__ m, MCArgs g, int64_t *__restrict__ bcounts) {
    int64_t blk = blockIdx.x;
    int64_t nblocks = gridDim.x;
    __shared__ int64_t lds[4];
    for (; blk * MC_CHUNK < g.n; blk += nblocks) {
        int64_t base = blk * MC_CHUNK;
        int64_t acc = 0;
        for (int j = 0; j < MC_ITEMS; ++j) {
            int64_t i = base + j * SCAN_THREADS + threadIdx.x;
            if (i < g.n && m[mc_addr(g, i, g.mstr)] != 0) ++acc;
        }
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0)
            bcounts[blk] = lds[0] + lds[1] + lds[2] + lds[3];
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(256) void mask_write_k(
    const T *__restrict__ a, const uint8_t *__restrict__ m,
    T *__restrict__ out, MCArgs g, const int64_t *__restrict__ bexcl) {
    // Everything is staged through LDS so HBM sees only coalesced
    // streams: values+mask in, the block-compacted run out (the naive
    // per-thread version's global writes were data-dependent partial
    // lines: measured 0.58 TB/s).  Thread t owns elements
    // [t*ITEMS, t*ITEMS+ITEMS) of the chunk, so the intra-chunk
    // exclusive scan of per-thread counts preserves C order.
    __shared__ T vals[MC_CHUNK + SCAN_THREADS];
    __shared__ T outbuf[MC_CHUNK];
    __shared__ unsigned char msk[MC_CHUNK + SCAN_THREADS];
    __shared__ int64_t wsum[4];
    int64_t blk = blockIdx.x;
    int64_t nblocks = gridDim.x;
    for (; blk * MC_CHUNK < g.n; blk += nblocks) {
        int64_t b0 = blk * MC_CHUNK;
        for (int j = 0; j < MC_ITEMS; ++j) {
            int64_t k = j * SCAN_THREADS + threadIdx.x;
            int64_t i = b0 + k;
            if (i < g.n) {
                msk[LIDX(k)] = m[mc_addr(g, i, g.mstr)];
                vals[LIDX(k)] = a[mc_addr(g, i, g.astr)];
            } else {
                msk[LIDX(k)] = 0;
            }
        }
        __syncthreads();
        int64_t l0 = (int64_t)threadIdx.x * MC_ITEMS;
        int64_t s = 0;
        for (int j = 0; j < MC_ITEMS; ++j)
            s += msk[LIDX(l0 + j)] != 0;
        int64_t x = s;
        int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
        for (int off = 1; off < 64; off <<= 1) {
            int64_t y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        if (lane == 63) wsum[wid] = x;
        __syncthreads();
        int64_t wbase = 0;
        for (int w = 0; w < wid; ++w) wbase += wsum[w];
        int64_t pos = wbase + x - s;        // block-local compacted index
        for (int j = 0; j < MC_ITEMS; ++j)
            if (msk[LIDX(l0 + j)] != 0) outbuf[pos++] = vals[LIDX(l0 + j)];
        int64_t btotal = 0;
        for (int w = 0; w < 4; ++w) btotal += wsum[w];
        __syncthreads();
        int64_t obase = bexcl[blk];
        for (int64_t k = threadIdx.x; k < btotal; k += SCAN_THREADS)
            out[obase + k] = outbuf[k];
        __syncthreads();
    }
}

template <typename T>
int mask_compact_launch(uintptr_t stream, const void *a, const void *m,
                        void *out, const MCArgs &g, void *bcounts,
                        int64_t nchunks, int phase) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int64_t grid = nchunks < 2048 ? nchunks : 2048;
    if (grid < 1) grid = 1;
    if (phase == 1) {
        if (g.nd == 1 && g.mstr[0] == 1
            && (reinterpret_cast<uintptr_t>(m) & 7) == 0) {
            hipLaunchKernelGGL(mask_count_vec_k, dim3((unsigned)grid),
                               dim3(SCAN_THREADS), 0, st,
                               static_cast<const uint8_t *>(m), g.n,
                               static_cast<int64_t *>(bcounts));
        } else {
            hipLaunchKernelGGL(mask_count_k, dim3((unsigned)grid),
                               dim3(SCAN_THREADS), 0, st,
                               static_cast<const uint8_t *>(m), g,
                               static_cast<int64_t *>(bcounts));
        }
    } else {
        hipLaunchKernelGGL((mask_write_k<T>), dim3((unsigned)grid),
                           dim3(SCAN_THREADS), 0, st,
                           static_cast<const T *>(a),
                           static_cast<const uint8_t *>(m),
                           static_cast<T *>(out), g,
                           static_cast<const int64_t *>(bcounts));
    }
    return launched("mask_compact");
}

}  // namespace

// chunk sizes the host sizes bsums / bcounts by
extern "C" int rt_scan_chunk(void) { return SCAN_CHUNK; }
extern "C" int rt_mask_chunk(void) { return MC_CHUNK; }

// phase 1: bcounts[c] = selected count of chunk c (nchunks =
// ceil(n / rt_mask_chunk()) int64 slots, 2048-element chunks).  Phase 2 is
// rt_cumsum(phase=2, dtype=2) on bcounts.  Phase 3: ordered write into
// dense `out`.  a/m pointers are pre-offset by the caller; strides/shape
// describe the local box.  dtype: any rt_dtype.
extern "C" int rt_mask_compact(uintptr_t stream, const void *a,
                               const void *m, void *out, int nd,
                               const int64_t *shape,
                               const int64_t *a_strides,
                               const int64_t *m_strides, void *bcounts,
                               int64_t nchunks, int dtype, int phase) {
    MCArgs g;
    if (box_extents("rt_mask_compact", nd, 1, shape, a_strides, m_strides,
                    &g.n))
        return 1;
    if (dtype < RT_F64 || dtype > RT_U8)
        return fail("rt_mask_compact", "bad dtype");
    if (phase != 1 && phase != 3)
        return fail("rt_mask_compact", "bad phase (1 or 3; phase 2 is "
                                       "rt_cumsum)");
    if (g.n == 0) return 0;
    // every chunk of n writes (phase 1) or reads (phase 3) its bcounts slot
    if (nchunks != (g.n + MC_CHUNK - 1) / MC_CHUNK)
        return fail("rt_mask_compact", "nchunks is not ceil(n / chunk)");
    if (!m) return fail("rt_mask_compact", "NULL m");
    if (!bcounts) return fail("rt_mask_compact", "NULL bcounts");
    if (phase == 3 && (!a || !out))
        return fail("rt_mask_compact", "NULL a/out");
    g.nd = nd;
    fill_geom(nd, shape, g.shape, a_strides, g.astr, m_strides, g.mstr);
    return dtype_dispatch<7>("rt_mask_compact", dtype, [&](auto t) {
        return mask_compact_launch<decltype(t)>(stream, a, m, out, g, bcounts,
                                                nchunks, phase);
    });
}

// ---------------------------------------------------------------------------
// axis-wise cumulative sum over the rank's local box (the
// N-D/axis half of the reference's scumulative, ramba/ramba.py:10057-10171 +
// scumulative_worker 3378-3440).  Local inclusive scan along `axis`, line
// totals into a dense slab; the cross-rank fixup is the host runtime's job
// (slab exchange + broadcast add via rt_combine_box with stride 0 on the
// scan axis — replaces the reference's sequential worker relay chain).
// Two mappings: axis != last -> one thread per line, serial walk, loads
// coalesced across threads; axis == last -> one wave per line, shfl_up
// segment scans with a carried prefix.
// ---------------------------------------------------------------------------

namespace {

struct ASArgs {
    int64_t len;        // shape[axis]
    int64_t nlines;     // product of the other axes
    int64_t lshape[3];  // line-index space (C order, axis removed)
    int64_t istr[3];    // in strides over the line space
    int64_t ostr[3];    // out strides over the line space
    int64_t istr_ax, ostr_ax;
    int nld;            // line-space ndim (nd - 1)
};

__device__ __forceinline__ void as_addr(const ASArgs &g, int64_t line,
                                        int64_t &ioff, int64_t &ooff) {
    int64_t rem = line;
    ioff = 0;
    ooff = 0;
    for (int d = g.nld - 1; d >= 0; --d) {
        int64_t idx = rem % g.lshape[d];
        rem /= g.lshape[d];
        ioff += idx * g.istr[d];
        ooff += idx * g.ostr[d];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void axis_scan_lines_k(
    const T *__restrict__ in, T *__restrict__ out,
    T *__restrict__ totals, ASArgs g) {
    int64_t line = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; line < g.nlines; line += stride) {
        int64_t ioff, ooff;
        as_addr(g, line, ioff, ooff);
        T acc = (T)0;
        for (int64_t k = 0; k < g.len; ++k) {
            acc += in[ioff + k * g.istr_ax];
            out[ooff + k * g.ostr_ax] = acc;
        }
        totals[line] = acc;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void axis_scan_waves_k(
    const T *__restrict__ in, T *__restrict__ out,
    T *__restrict__ totals, ASArgs g) {
    int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    int lane = threadIdx.x & 63;
    for (int64_t line = wave; line < g.nlines; line += nwaves) {
        int64_t ioff, ooff;
        as_addr(g, line, ioff, ooff);
        T carry = (T)0;
        for (int64_t base = 0; base < g.len; base += 64) {
            int64_t k = base + lane;
            T x = k < g.len ? in[ioff + k * g.istr_ax] : (T)0;
            for (int off = 1; off < 64; off <<= 1) {
                T y = __shfl_up(x, off, 64);
                if (lane >= off) x += y;
            }
            x += carry;
            if (k < g.len) out[ooff + k * g.ostr_ax] = x;
            carry = __shfl(x, 63, 64);
        }
        if (lane == 0) totals[line] = carry;
    }
}

// chunked variant for axis != last with FEW lines: nlines threads alone
// starve the chip (16384 columns = 64 workgroups: measured 0.17 TB/s), so
// the scan axis is split into `nchunks` ranges — k1 scans each (line,
// chunk) range locally and records its sum, k2 turns the per-chunk sums
// into exclusive offsets per line (and writes the final line totals), k3
// adds the offsets back.  3 passes over out ≈ 32 B/elem vs 16, but the
// chip is full.
template <typename T>
__global__ __launch_bounds__(256) void axis_scan_ck1(
    const T *__restrict__ in, T *__restrict__ out, T *__restrict__ tot2,
    ASArgs g, int64_t nchunks, int64_t clen) {
    int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t work = g.nlines * nchunks;
    for (; w < work; w += stride) {
        int64_t line = w % g.nlines;
        int64_t c = w / g.nlines;
        int64_t k0 = c * clen;
        int64_t k1 = k0 + clen < g.len ? k0 + clen : g.len;
        int64_t ioff, ooff;
        as_addr(g, line, ioff, ooff);
        T acc = (T)0;
        for (int64_t k = k0; k < k1; ++k) {
            acc += in[ioff + k * g.istr_ax];
            out[ooff + k * g.ostr_ax] = acc;
        }
        tot2[c * g.nlines + line] = acc;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void axis_scan_ck2(
    T *__restrict__ tot2, T *__restrict__ totals, int64_t nlines,
    int64_t nchunks) {
    int64_t line = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; line < nlines; line += stride) {
        T run = (T)0;
        for (int64_t c = 0; c < nchunks; ++c) {
            T t = tot2[c * nlines + line];
            tot2[c * nlines + line] = run;
            run += t;
        }
        totals[line] = run;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void axis_scan_ck3(
    T *__restrict__ out, const T *__restrict__ tot2, ASArgs g,
    int64_t nchunks, int64_t clen) {
    // chunks 1.. only; chunk 0's offset is zero
    int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t work = g.nlines * (nchunks - 1);
    for (; w < work; w += stride) {
        int64_t line = w % g.nlines;
        int64_t c = 1 + w / g.nlines;
        T off = tot2[c * g.nlines + line];
        int64_t k0 = c * clen;
        int64_t k1 = k0 + clen < g.len ? k0 + clen : g.len;
        int64_t ioff, ooff;
        as_addr(g, line, ioff, ooff);
        for (int64_t k = k0; k < k1; ++k)
            out[ooff + k * g.ostr_ax] += off;
    }
}

template <typename T>
int axis_scan_chunked_launch(uintptr_t stream, const void *in, void *out,
                             void *totals, void *tot2, const ASArgs &g,
                             int64_t nchunks) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int64_t clen = (g.len + nchunks - 1) / nchunks;
    int64_t work = g.nlines * nchunks;
    int64_t blocks = (work + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL((axis_scan_ck1<T>), dim3((unsigned)blocks), dim3(256),
                       0, st, static_cast<const T *>(in),
                       static_cast<T *>(out), static_cast<T *>(tot2), g,
                       nchunks, clen);
    int64_t b2 = (g.nlines + 255) / 256;
    if (b2 > 4096) b2 = 4096;
    if (b2 < 1) b2 = 1;
    hipLaunchKernelGGL((axis_scan_ck2<T>), dim3((unsigned)b2), dim3(256), 0,
                       st, static_cast<T *>(tot2), static_cast<T *>(totals),
                       g.nlines, nchunks);
    if (nchunks > 1)
        hipLaunchKernelGGL((axis_scan_ck3<T>), dim3((unsigned)blocks),
                           dim3(256), 0, st, static_cast<T *>(out),
                           static_cast<const T *>(tot2), g, nchunks, clen);
    return launched("axis_scan chunked");
}

template <typename T>
int axis_scan_launch(uintptr_t stream, const void *in, void *out,
                     void *totals, const ASArgs &g, int waves) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int64_t work = waves ? g.nlines * 64 : g.nlines;
    int64_t blocks = (work + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    if (waves)
        hipLaunchKernelGGL((axis_scan_waves_k<T>), dim3((unsigned)blocks),
                           dim3(256), 0, st, static_cast<const T *>(in),
                           static_cast<T *>(out), static_cast<T *>(totals),
                           g);
    else
        hipLaunchKernelGGL((axis_scan_lines_k<T>), dim3((unsigned)blocks),
                           dim3(256), 0, st, static_cast<const T *>(in),
                           static_cast<T *>(out), static_cast<T *>(totals),
                           g);
    return launched("axis_scan");
}

}  // namespace

// in/out pre-offset to the box origin; shape/strides over the FULL local
// box (nd dims, nd 2..4); totals: dense C-order slab of the line space.
// dtype: RT_F64 .. RT_I32.  nchunks > 1 selects the chunked
// variant (axis != last with few lines); tot2 then holds
// nchunks × nlines scratch.
extern "C" int rt_axis_scan(uintptr_t stream, const void *in, void *out,
                            void *totals, int nd, const int64_t *shape,
                            const int64_t *in_strides,
                            const int64_t *out_strides, int axis,
                            int dtype, void *tot2, int64_t nchunks) {
    int64_t nbox = 0;
    if (box_extents("rt_axis_scan", nd, 2, shape, in_strides, out_strides,
                    &nbox))
        return 1;
    if (axis < 0 || axis >= nd)
        return fail("rt_axis_scan", "axis out of range");
    if (dtype < RT_F64 || dtype > RT_I32)
        return fail("rt_axis_scan", "bad dtype");
    if (nchunks < 1) return fail("rt_axis_scan", "nchunks < 1");
    if (nchunks > 1 && !tot2)
        return fail("rt_axis_scan", "nchunks > 1 needs tot2");
    if (nbox == 0) return 0;
    if (!in || !out || !totals)
        return fail("rt_axis_scan", "NULL in/out/totals");
    ASArgs g;
    g.len = shape[axis];
    g.istr_ax = in_strides[axis];
    g.ostr_ax = out_strides[axis];
    g.nld = 0;
    g.nlines = 1;
    for (int d = 0; d < nd; ++d) {
        if (d == axis) continue;
        g.lshape[g.nld] = shape[d];
        g.istr[g.nld] = in_strides[d];
        g.ostr[g.nld] = out_strides[d];
        g.nlines *= shape[d];
        ++g.nld;
    }
    for (int d = g.nld; d < 3; ++d) {
        g.lshape[d] = 1;
        g.istr[d] = 0;
        g.ostr[d] = 0;
    }
    if (nchunks > (1LL << 46) / g.nlines)
        return fail("rt_axis_scan", "nchunks * lines too large");
    int waves = (axis == nd - 1) ? 1 : 0;
    return dtype_dispatch<4>("rt_axis_scan", dtype, [&](auto t) {
        using T = decltype(t);
        if (nchunks > 1)
            return axis_scan_chunked_launch<T>(stream, in, out, totals, tot2,
                                               g, nchunks);
        return axis_scan_launch<T>(stream, in, out, totals, g, waves);
    });
}

// ---------------------------------------------------------------------------
// flat-order gather/scatter between a strided local box and a dense buffer
// (reshape data movement; the reference's per-element flat-index remap
// worker, ramba/ramba.py:2409-2492, becomes interval exchange + these two
// kernels).  flat0/n select a C-order flat subrange of the box.
// ---------------------------------------------------------------------------

namespace {

struct FlatArgs {
    int64_t n;          // elements in the subrange
    int64_t flat0;      // first flat index within the box
    int64_t shape[4];
    int64_t str[4];     // element strides of the boxed side
    int nd;
};

// row-wise mapping: one div/mod chain per ROW per block instead of per
// element (int64 division is ~100 cycles on CDNA4 and dominated the
// naive per-element version: measured 0.40 TB/s -> row-wise streams).
// A "row" is one span of the last axis; threads sweep it coalesced.
template <typename T, int SCATTER>
__global__ __launch_bounds__(256) void flat_copy_1d_kernel(
    T *__restrict__ boxed, T *__restrict__ dense, int64_t flat0,
    int64_t n, int64_t str) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        if (SCATTER) boxed[(flat0 + i) * str] = dense[i];
        else dense[i] = boxed[(flat0 + i) * str];
    }
}

template <typename T, int SCATTER>
__global__ __launch_bounds__(256) void flat_copy_kernel(
    T *__restrict__ boxed, T *__restrict__ dense, FlatArgs g,
    int64_t cpr /* column chunks per row (fills the chip when rows are
                   few and the inner axis is huge) */) {
    const int64_t inner = g.shape[g.nd - 1];
    const int64_t sin_ = g.str[g.nd - 1];
    const int64_t row_lo = g.flat0 / inner;
    const int64_t row_hi = (g.flat0 + g.n - 1) / inner;   // inclusive
    const int64_t span = (inner + cpr - 1) / cpr;
    for (int64_t b = blockIdx.x;; b += gridDim.x) {
        int64_t row = row_lo + b / cpr;
        if (row > row_hi) break;
        int64_t chunk = b % cpr;
        // outer-coordinate offset for this row (one divmod chain)
        int64_t rem = row, off = 0;
        for (int d = g.nd - 2; d >= 0; --d) {
            int64_t idx = rem % g.shape[d];
            rem /= g.shape[d];
            off += idx * g.str[d];
        }
        int64_t fbase = row * inner;
        int64_t c0 = fbase < g.flat0 ? g.flat0 - fbase : 0;
        int64_t c1 = fbase + inner > g.flat0 + g.n ? g.flat0 + g.n - fbase
                                                   : inner;
        if (chunk * span > c0) c0 = chunk * span;
        if ((chunk + 1) * span < c1) c1 = (chunk + 1) * span;
        for (int64_t c = c0 + threadIdx.x; c < c1; c += blockDim.x) {
            int64_t di = fbase + c - g.flat0;
            if (SCATTER) boxed[off + c * sin_] = dense[di];
            else dense[di] = boxed[off + c * sin_];
        }
    }
}

template <typename T>
int flat_copy_launch(uintptr_t stream, void *boxed, void *dense,
                     const FlatArgs &g, int scatter) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (g.nd == 1) {
        int64_t blocks = (g.n + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        if (blocks < 1) blocks = 1;
        if (scatter)
            hipLaunchKernelGGL((flat_copy_1d_kernel<T, 1>),
                               dim3((unsigned)blocks), dim3(256), 0, st,
                               static_cast<T *>(boxed),
                               static_cast<T *>(dense), g.flat0, g.n,
                               g.str[0]);
        else
            hipLaunchKernelGGL((flat_copy_1d_kernel<T, 0>),
                               dim3((unsigned)blocks), dim3(256), 0, st,
                               static_cast<T *>(boxed),
                               static_cast<T *>(dense), g.flat0, g.n,
                               g.str[0]);
        return launched("flat_copy");
    }
    int64_t inner = g.shape[g.nd - 1];
    int64_t rows = (g.n + inner - 1) / inner + 1;
    int64_t cpr = 1;
    if (rows < 2048) {
        cpr = 2048 / rows;
        int64_t maxc = (inner + 65535) / 65536;
        if (cpr > maxc) cpr = maxc;
        if (cpr < 1) cpr = 1;
    }
    int64_t blocks = rows * cpr < 4096 ? rows * cpr : 4096;
    if (blocks < 1) blocks = 1;
    if (scatter)
        hipLaunchKernelGGL((flat_copy_kernel<T, 1>), dim3((unsigned)blocks),
                           dim3(256), 0, st, static_cast<T *>(boxed),
                           static_cast<T *>(dense), g, cpr);
    else
        hipLaunchKernelGGL((flat_copy_kernel<T, 0>), dim3((unsigned)blocks),
                           dim3(256), 0, st, static_cast<T *>(boxed),
                           static_cast<T *>(dense), g, cpr);
    return launched("flat_copy");
}

}  // namespace

// boxed pointer is pre-offset to the box origin; scatter=0 gathers the
// flat subrange [flat0, flat0+n) of the box into dense, scatter=1 writes
// dense back into that subrange.
extern "C" int rt_flat_copy(uintptr_t stream, void *boxed, void *dense,
                            int nd, const int64_t *shape,
                            const int64_t *strides, int64_t flat0,
                            int64_t n, int elemsize, int scatter) {
    int64_t nbox = 0;
    if (box_extents("rt_flat_copy", nd, 1, shape, strides, strides, &nbox))
        return 1;
    if (elemsize != 1 && elemsize != 2 && elemsize != 4 && elemsize != 8)
        return fail("rt_flat_copy", "bad elemsize");
    if (scatter != 0 && scatter != 1)
        return fail("rt_flat_copy", "bad scatter (0 or 1)");
    if (flat0 < 0) return fail("rt_flat_copy", "negative flat0");
    if (n < 0) return fail("rt_flat_copy", "negative n");
    if (flat0 > nbox || n > nbox - flat0)
        return fail("rt_flat_copy", "flat0 + n past the end of the box");
    if (n == 0) return 0;
    if (!boxed || !dense) return fail("rt_flat_copy", "NULL boxed/dense");
    FlatArgs g;
    g.nd = nd;
    g.n = n;
    g.flat0 = flat0;
    fill_geom(nd, shape, g.shape, strides, g.str);
    switch (elemsize) {
        case 1: return flat_copy_launch<uint8_t>(stream, boxed, dense, g,
                                                 scatter);
        case 2: return flat_copy_launch<uint16_t>(stream, boxed, dense, g,
                                                  scatter);
        case 4: return flat_copy_launch<uint32_t>(stream, boxed, dense, g,
                                                  scatter);
        case 8: return flat_copy_launch<uint64_t>(stream, boxed, dense, g,
                                                  scatter);
        default:
            set_error("rt_flat_copy: bad elemsize");
            return 1;
    }
}

// ---------------------------------------------------------------------------
// indexed row gather / placement (integer-array getitem and take; the
// reference's all2all getitem worker, ramba/ramba.py:3960, moves per-element
// lists — here the unit is a whole ROW of the axis-0-split source).
//     dst[dr(k)] = src[sr(k)]   for k in [0, n)
// A row is a strided box of up to 3 inner axes (shard containers pad the
// innermost axis, message buffers are dense).  Every row number is checked
// against src_nrows / dst_nrows BEFORE an address is formed; a bad row is
// skipped and counted in *bad.
// ---------------------------------------------------------------------------

namespace {

struct TakeArgs {
    int64_t n, src_nrows, dst_nrows;
    int64_t src_rs, dst_rs;     // row strides, in kernel access units
    int64_t sstr[3], dstr[3];   // inner strides (outer..inner), same units
    uint32_t shp[3];            // inner extents, left-padded with 1
    int nd;                     // real inner axes (0..3)
};

// src row for entry k (a negative source row wraps once, NumPy style) and
// dst row; false when either is out of range
__device__ __forceinline__ bool take_rows_of(const TakeArgs &g,
                                             const int64_t *sr,
                                             const int64_t *dr, int64_t k,
                                             int64_t &s, int64_t &d) {
    s = sr ? sr[k] : k;
    if (s < 0) s += g.src_nrows;
    d = dr ? dr[k] : k;
    return (uint64_t)s < (uint64_t)g.src_nrows
        && (uint64_t)d < (uint64_t)g.dst_nrows;
}

__device__ __forceinline__ void take_inner_off(const TakeArgs &g, uint32_t j,
                                               int64_t &os, int64_t &od) {
    // j = flat C-order position inside the row (in access units)
    if (g.nd <= 1) {
        os = (int64_t)j * g.sstr[2];
        od = (int64_t)j * g.dstr[2];
        return;
    }
    uint32_t q = j / g.shp[2], c2 = j - q * g.shp[2];
    uint32_t c0 = q / g.shp[1], c1 = q - c0 * g.shp[1];
    os = c0 * g.sstr[0] + c1 * g.sstr[1] + c2 * g.sstr[2];
    od = c0 * g.dstr[0] + c1 * g.dstr[1] + c2 * g.dstr[2];
}

// NARROW regime: one thread per output element.  Consecutive threads take
// consecutive entries k (ONE: the 1-D case, row = one element) or
// consecutive elements of a row, so the index load and the dense side are
// coalesced.  The only 64-bit division is block-uniform.
template <typename T, bool ONE>
__global__ __launch_bounds__(256) void take_narrow_kernel(
    T *__restrict__ dst, const T *__restrict__ src,
    const int64_t *__restrict__ sr, const int64_t *__restrict__ dr,
    TakeArgs g, uint32_t re, unsigned int *bad) {
    const int64_t total = g.n * (int64_t)re;
    const int64_t nblk = (total + 255) / 256;
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
        const int64_t base = b * 256;
        int64_t k;
        uint32_t j = 0;
        if (ONE) {
            k = base + threadIdx.x;
        } else {
            const int64_t k0 = base / re;
            const uint32_t t = (uint32_t)(base - k0 * re) + threadIdx.x;
            const uint32_t dk = t / re;
            j = t - dk * re;
            k = k0 + dk;
        }
        if (k >= g.n) continue;
        int64_t s, d;
        if (!take_rows_of(g, sr, dr, k, s, d)) {
            if (j == 0 && bad) atomicAdd(bad, 1u);
            continue;
        }
        int64_t os = 0, od = 0;
        if (!ONE) take_inner_off(g, j, os, od);
        dst[d * g.dst_rs + od] = src[s * g.src_rs + os];
    }
}

// WIDE regime: one wave per destination row, 4 rows in flight per wave
// (the shape the MI355X guide measured for random whole rows); lanes sweep
// the row in access units V — 16-byte uint4 when the geometry allows it,
// one element otherwise.
template <typename V>
__global__ __launch_bounds__(256) void take_wide_kernel(
    V *__restrict__ dst, const V *__restrict__ src,
    const int64_t *__restrict__ sr, const int64_t *__restrict__ dr,
    TakeArgs g, uint32_t units, unsigned int *bad) {
    const uint32_t lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t ngroups = (g.n + 3) / 4;
    for (int64_t grp = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
         grp < ngroups; grp += nwaves) {
        int64_t so[4], dof[4];
        bool ok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t k = grp * 4 + r;
            so[r] = dof[r] = 0;
            ok[r] = false;
            if (k < g.n) {
                int64_t s, d;
                ok[r] = take_rows_of(g, sr, dr, k, s, d);
                if (ok[r]) {
                    so[r] = s * g.src_rs;
                    dof[r] = d * g.dst_rs;
                } else if (lane == 0 && bad) {
                    atomicAdd(bad, 1u);
                }
            }
        }
        for (uint32_t u = lane; u < units; u += 64) {
            int64_t os, od;
            take_inner_off(g, u, os, od);
            V v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (ok[r]) v[r] = src[so[r] + os];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (ok[r]) dst[dof[r] + od] = v[r];
        }
    }
}

// Regime choice (host): rows under 256 B go one thread per element — a
// wave per row would leave most lanes idle; wider rows go one wave per row,
// with 16-byte accesses iff the innermost extent, every stride (in bytes)
// and both base pointers are multiples of 16.
enum { TAKE_NARROW = 0, TAKE_WIDE_VEC = 1, TAKE_WIDE_SCALAR = 2 };

int take_regime(const void *dst, const void *src, int nd_inner,
                const int64_t *inner_shape, const int64_t *src_strides,
                const int64_t *dst_strides, int64_t src_row_stride,
                int64_t dst_row_stride, int elemsize) {
    int64_t re = 1;
    for (int d = 0; d < nd_inner; ++d) re *= inner_shape[d];
    if (re * elemsize < 256) return TAKE_NARROW;
    const int64_t es = elemsize;
    bool vec = nd_inner >= 1
        && (inner_shape[nd_inner - 1] * es) % 16 == 0
        && src_strides[nd_inner - 1] == 1 && dst_strides[nd_inner - 1] == 1
        && (src_row_stride * es) % 16 == 0 && (dst_row_stride * es) % 16 == 0
        && reinterpret_cast<uintptr_t>(dst) % 16 == 0
        && reinterpret_cast<uintptr_t>(src) % 16 == 0;
    for (int d = 0; vec && d < nd_inner - 1; ++d)
        vec = (src_strides[d] * es) % 16 == 0
            && (dst_strides[d] * es) % 16 == 0;
    return vec ? TAKE_WIDE_VEC : TAKE_WIDE_SCALAR;
}

int take_validate(const void *dst, const void *src, int64_t n, int nd_inner,
                  const int64_t *inner_shape, const int64_t *src_strides,
                  const int64_t *dst_strides, int elemsize) {
    if (elemsize != 1 && elemsize != 2 && elemsize != 4 && elemsize != 8) {
        set_error("rt_take_rows: bad elemsize");
        return 1;
    }
    if (nd_inner < 0 || nd_inner > 3) {
        set_error("rt_take_rows: nd_inner out of range");
        return 1;
    }
    if (n < 0) {
        set_error("rt_take_rows: negative n");
        return 1;
    }
    if (n > 0 && (dst == nullptr || src == nullptr)) {
        set_error("rt_take_rows: NULL dst/src");
        return 1;
    }
    if (nd_inner > 0 && (!inner_shape || !src_strides || !dst_strides)) {
        set_error("rt_take_rows: NULL inner geometry");
        return 1;
    }
    int64_t re = 1;
    for (int d = 0; d < nd_inner; ++d) {
        if (inner_shape[d] < 0 || inner_shape[d] >= (1LL << 31)) {
            set_error("rt_take_rows: inner extent out of range");
            return 1;
        }
        re *= inner_shape[d];
        if (re >= (1LL << 31)) {
            set_error("rt_take_rows: row too large");
            return 1;
        }
    }
    return 0;
}

template <typename T>
int take_launch(uintptr_t stream, void *dst, const void *src,
                const int64_t *sr, const int64_t *dr, TakeArgs g,
                int64_t re, int regime, void *bad) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned int *badp = static_cast<unsigned int *>(bad);
    if (regime == TAKE_NARROW) {
        int64_t blocks = (g.n * re + 255) / 256;
        if (blocks > 65536) blocks = 65536;
        if (re == 1)
            hipLaunchKernelGGL((take_narrow_kernel<T, true>),
                               dim3((unsigned)blocks), dim3(256), 0, st,
                               static_cast<T *>(dst),
                               static_cast<const T *>(src), sr, dr, g,
                               (uint32_t)re, badp);
        else
            hipLaunchKernelGGL((take_narrow_kernel<T, false>),
                               dim3((unsigned)blocks), dim3(256), 0, st,
                               static_cast<T *>(dst),
                               static_cast<const T *>(src), sr, dr, g,
                               (uint32_t)re, badp);
    } else {
        // 4 waves per block, 4 rows per wave pass; 16 waves per CU on
        // 256 CUs = 1024 resident blocks, the rest by grid stride
        int64_t blocks = (g.n + 15) / 16;
        if (blocks > 4096) blocks = 4096;
        if (regime == TAKE_WIDE_VEC) {
            const int64_t per = 16 / (int64_t)sizeof(T);
            TakeArgs v = g;
            v.src_rs /= per;
            v.dst_rs /= per;
            for (int d = 0; d < 2; ++d) {
                v.sstr[d] /= per;
                v.dstr[d] /= per;
            }
            v.shp[2] = (uint32_t)(g.shp[2] / per);
            hipLaunchKernelGGL((take_wide_kernel<uint4>),
                               dim3((unsigned)blocks), dim3(256), 0, st,
                               static_cast<uint4 *>(dst),
                               static_cast<const uint4 *>(src), sr, dr, v,
                               (uint32_t)(re / per), badp);
        } else {
            hipLaunchKernelGGL((take_wide_kernel<T>),
                               dim3((unsigned)blocks), dim3(256), 0, st,
                               static_cast<T *>(dst),
                               static_cast<const T *>(src), sr, dr, g,
                               (uint32_t)re, badp);
        }
    }
    return launched("take_rows");
}

}  // namespace

// Which kernel rt_take_rows would run for this geometry: 0 = narrow (thread
// per element), 1 = wide with 16-byte accesses, 2 = wide scalar; -1 on bad
// arguments.  Pure host arithmetic (pointers are only tested for alignment).
extern "C" int rt_take_regime(const void *dst, const void *src, int nd_inner,
                              const int64_t *inner_shape,
                              const int64_t *src_strides,
                              const int64_t *dst_strides,
                              int64_t src_row_stride, int64_t dst_row_stride,
                              int elemsize) {
    if (take_validate(dst, src, 0, nd_inner, inner_shape, src_strides,
                      dst_strides, elemsize))
        return -1;
    return take_regime(dst, src, nd_inner, inner_shape, src_strides,
                       dst_strides, src_row_stride, dst_row_stride,
                       elemsize);
}

// dst / src point at row 0 (pre-offset to the core origin); strides are in
// elements.  src_rows / dst_rows are device int64[n] or NULL (identity).
extern "C" int rt_take_rows(uintptr_t stream, void *dst, const void *src,
                            const int64_t *src_rows, const int64_t *dst_rows,
                            int64_t n, int64_t src_nrows, int64_t dst_nrows,
                            int nd_inner, const int64_t *inner_shape,
                            const int64_t *src_strides,
                            const int64_t *dst_strides,
                            int64_t src_row_stride, int64_t dst_row_stride,
                            int elemsize, void *bad) {
    if (take_validate(dst, src, n, nd_inner, inner_shape, src_strides,
                      dst_strides, elemsize))
        return 1;
    if (n == 0) return 0;
    TakeArgs g;
    g.n = n;
    g.src_nrows = src_nrows;
    g.dst_nrows = dst_nrows;
    g.src_rs = src_row_stride;
    g.dst_rs = dst_row_stride;
    g.nd = nd_inner;
    int64_t re = 1;
    for (int d = 0; d < 3; ++d) {
        const int s = d - (3 - nd_inner);
        g.shp[d] = s >= 0 ? (uint32_t)inner_shape[s] : 1u;
        g.sstr[d] = s >= 0 ? src_strides[s] : 0;
        g.dstr[d] = s >= 0 ? dst_strides[s] : 0;
        re *= g.shp[d];
    }
    if (re == 0) return 0;
    const int regime = take_regime(dst, src, nd_inner, inner_shape,
                                   src_strides, dst_strides, src_row_stride,
                                   dst_row_stride, elemsize);
    switch (elemsize) {
        case 1: return take_launch<uint8_t>(stream, dst, src, src_rows,
                                            dst_rows, g, re, regime, bad);
        case 2: return take_launch<uint16_t>(stream, dst, src, src_rows,
                                             dst_rows, g, re, regime, bad);
        case 4: return take_launch<uint32_t>(stream, dst, src, src_rows,
                                             dst_rows, g, re, regime, bad);
        default: return take_launch<uint64_t>(stream, dst, src, src_rows,
                                              dst_rows, g, re, regime, bad);
    }
}

// ---------------------------------------------------------------------------
// argmax / argmin / nanargmax / nanargmin: (value, index) pair reductions.
// The reference only lists these as to-do (ramba/ramba.py:10288).
//
// Every kernel carries a pair through its tree and merges with the one
// comparator of include/ramba_argcmp.h.  An element's index is always
// derived from its coordinates in the box —
//     idx = idx0 + sum_d coord_d * mult_d
// (mult = 1 on the reduced axis for an axis reduction, the view shape's C
// strides for the flat one; idx0 places the rank's box in the global view)
// — never from a running counter, so a reversed, stepped or transposed
// operand reports view order.  No atomics: the pair order is total, the
// result is the same pair whatever the grouping.  No kernel forms an
// address from data; extents, strides and the dtype code are validated on
// the host side of each entry before anything is launched.
// ---------------------------------------------------------------------------

#include "../../include/ramba_argcmp.h"

namespace {

// blocks of the flat stage 1 (256 CUs x 8 blocks, the memory-bound grid
// cap); each block leaves one pair for stage 2
enum { ARG_GRID_CAP = 2048 };

template <typename T>
__device__ __forceinline__ T arg_shfl(T v, int d) {
    if constexpr (sizeof(T) == 8) {
        long long b;
        __builtin_memcpy(&b, &v, 8);
        b = __shfl_down(b, d);
        T r;
        __builtin_memcpy(&r, &b, 8);
        return r;
    } else if constexpr (sizeof(T) == 4) {
        int b;
        __builtin_memcpy(&b, &v, 4);
        b = __shfl_down(b, d);
        T r;
        __builtin_memcpy(&r, &b, 4);
        return r;
    } else {
        return (T)__shfl_down((int)v, d);
    }
}

template <typename T>
__device__ __forceinline__ void arg_take(T &bv, int64_t &bi, T v, int64_t i,
                                         int mx, int sk) {
    if (rt_arg_better<T>(v, i, bv, bi, mx, sk)) {
        bv = v;
        bi = i;
    }
}

// all 64 lanes take part; the wave's pair ends in lane 0
template <typename T>
__device__ __forceinline__ void arg_wave_reduce(T &bv, int64_t &bi, int mx,
                                                int sk) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const T ov = arg_shfl<T>(bv, d);
        const int64_t oi = arg_shfl<int64_t>(bi, d);
        arg_take<T>(bv, bi, ov, oi, mx, sk);
    }
}

// 256 threads = 4 waves: shuffles, then an LDS hand-off; the block's pair
// ends in thread 0
template <typename T>
__device__ __forceinline__ void arg_block_reduce(T &bv, int64_t &bi, int mx,
                                                 int sk) {
    __shared__ T sv[4];
    __shared__ int64_t si[4];
    arg_wave_reduce<T>(bv, bi, mx, sk);
    if ((threadIdx.x & 63) == 0) {
        sv[threadIdx.x >> 6] = bv;
        si[threadIdx.x >> 6] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < 4; ++k) arg_take<T>(bv, bi, sv[k], si[k], mx, sk);
}

// -- flat (all axes) ---------------------------------------------------------

struct ArgFlatArgs {
    int64_t nunits;          // load units in the box
    int64_t shp[4];          // extents, right-aligned; innermost in units
    int64_t str[4];          // strides in load units
    int64_t mult[4];         // index multiplier per ELEMENT coordinate
    int64_t idx0;
    int64_t tail0, tailn;    // 1-D 16-byte path: elements past the last unit
    int nd, is_max, skipna;
};

template <typename T, typename L>
__device__ __forceinline__ void arg_flat_addr(const ArgFlatArgs &a, int64_t u,
                                              int64_t &off, int64_t &ib) {
    constexpr int PER = sizeof(L) / sizeof(T);
    if (a.nd == 1) {
        off = u * a.str[3];
        ib = a.idx0 + u * PER * a.mult[3];
        return;
    }
    uint64_t rem = (uint64_t)u;
    off = 0;
    ib = a.idx0;
#pragma unroll
    for (int d = 3; d >= 0; --d) {
        const uint64_t q = rem / (uint64_t)a.shp[d];
        const int64_t c = (int64_t)(rem - q * (uint64_t)a.shp[d]);
        rem = q;
        off += c * a.str[d];
        ib += c * (d == 3 ? PER : 1) * a.mult[d];
    }
}

// In-thread accumulate of one load unit whose elements sit at indices ib,
// ib + step, ...: every thread walks its elements in increasing index
// order, so the comparator's LATER form applies (strictly better only) and
// the 64-bit index is formed only when an element is taken.  MX / SK are
// compile-time so the test folds.
template <typename T, typename L, int MX, int SK>
__device__ __forceinline__ void arg_unit_acc(const L &unit, int64_t ib,
                                             int64_t step, T &bv,
                                             int64_t &bi) {
    constexpr int PER = sizeof(L) / sizeof(T);
    T e[PER];
    __builtin_memcpy(e, &unit, sizeof(L));
#pragma unroll
    for (int j = 0; j < PER; ++j)
        if (rt_arg_better<T, true>(e[j], 0, bv, bi, MX, SK)) {
            bv = e[j];
            bi = ib + j * step;
        }
}

// run BODY<MX, SK> for the launch's (uniform) is_max / skipna
#define ARG_FLAGS(mx, sk, BODY)                                            \
    do {                                                                   \
        if (mx) {                                                          \
            if (sk) BODY(1, 1); else BODY(1, 0);                           \
        } else {                                                           \
            if (sk) BODY(0, 1); else BODY(0, 0);                           \
        }                                                                  \
    } while (0)

template <typename T, typename L, int MX, int SK>
__device__ __forceinline__ void arg_flat_walk(const T *__restrict__ in,
                                              const ArgFlatArgs &a, T &bv,
                                              int64_t &bi) {
    const L *src = reinterpret_cast<const L *>(in);
    const int64_t S = (int64_t)gridDim.x * 256;
    const int64_t step = a.mult[3];
    int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (; u + S < a.nunits; u += 2 * S) {
        int64_t o0, i0, o1, i1;
        arg_flat_addr<T, L>(a, u, o0, i0);
        arg_flat_addr<T, L>(a, u + S, o1, i1);
        const L x0 = src[o0];
        const L x1 = src[o1];
        arg_unit_acc<T, L, MX, SK>(x0, i0, step, bv, bi);
        arg_unit_acc<T, L, MX, SK>(x1, i1, step, bv, bi);
    }
    if (u < a.nunits) {
        int64_t o0, i0;
        arg_flat_addr<T, L>(a, u, o0, i0);
        const L x0 = src[o0];
        arg_unit_acc<T, L, MX, SK>(x0, i0, step, bv, bi);
    }
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < a.tailn)
        arg_unit_acc<T, T, MX, SK>(in[a.tail0 + t],
                                   a.idx0 + (a.tail0 + t) * step, step, bv,
                                   bi);
}

// Stage 1: grid-stride over the box's load units (L = uint4 when the
// innermost stride is 1 and everything is 16-byte aligned, else one
// element), two loads in flight per lane; one pair per block.
template <typename T, typename L>
__global__ __launch_bounds__(256) void arg_flat_s1(const T *__restrict__ in,
                                                   ArgFlatArgs a,
                                                   T *__restrict__ pv,
                                                   int64_t *__restrict__ pi) {
    T bv = T(0);
    int64_t bi = -1;
#define BODY(MX, SK) arg_flat_walk<T, L, MX, SK>(in, a, bv, bi)
    ARG_FLAGS(a.is_max, a.skipna, BODY);
#undef BODY
    arg_block_reduce<T>(bv, bi, a.is_max, a.skipna);
    if (threadIdx.x == 0) {
        pv[blockIdx.x] = bv;
        pi[blockIdx.x] = bi;
    }
}

// Stage 2: one block reduces the per-block pairs into the output pair
template <typename T>
__global__ __launch_bounds__(256) void arg_flat_s2(
    const T *__restrict__ pv, const int64_t *__restrict__ pi, int n,
    T *__restrict__ ov, int64_t *__restrict__ oi, int mx, int sk) {
    T bv = T(0);
    int64_t bi = -1;
    for (int k = threadIdx.x; k < n; k += 256)
        arg_take<T>(bv, bi, pv[k], pi[k], mx, sk);
    arg_block_reduce<T>(bv, bi, mx, sk);
    if (threadIdx.x == 0) {
        ov[0] = bv;
        oi[0] = bi;
    }
}

// 16-byte loads iff the innermost stride is 1, the first element is
// 16-byte aligned and, beyond 1-D, the innermost extent and every outer
// stride are whole units (1-D keeps a scalar tail instead)
bool arg_flat_vec(const void *in, int64_t in_off, int nd,
                  const int64_t *shape, const int64_t *strides, int es) {
    const int64_t per = 16 / es;
    if (strides[nd - 1] != 1) return false;
    if ((reinterpret_cast<uintptr_t>(in) + (uint64_t)(in_off * es)) % 16)
        return false;
    if (nd == 1) return shape[0] >= per;
    if (shape[nd - 1] % per) return false;
    for (int d = 0; d < nd - 1; ++d)
        if (strides[d] % per) return false;
    return true;
}

int arg_validate(const char *who, const void *in, int nd,
                 const int64_t *shape, const int64_t *strides, int dtype,
                 int64_t *n_out) {
    if (dtype < RT_F64 || dtype > RT_U8) {
        set_error(std::string(who) + ": bad dtype");
        return 1;
    }
    if (nd < 1 || nd > 4) {
        set_error(std::string(who) + ": nd out of range");
        return 1;
    }
    if (!in || !shape || !strides) {
        set_error(std::string(who) + ": NULL argument");
        return 1;
    }
    int64_t n = 1;
    for (int d = 0; d < nd; ++d) {
        if (shape[d] < 1 || shape[d] >= (1LL << 40)) {
            set_error(std::string(who) + ": extent out of range");
            return 1;
        }
        if (n > (1LL << 46) / shape[d]) {
            set_error(std::string(who) + ": box too large");
            return 1;
        }
        n *= shape[d];
    }
    *n_out = n;
    return 0;
}

template <typename T>
int arg_flat_launch(uintptr_t stream, const void *in, int64_t in_off, int nd,
                    const int64_t *shape, const int64_t *strides,
                    const int64_t *mult, int64_t idx0, int64_t n, bool vec,
                    int is_max, int skipna, void *sv, void *si, void *ov,
                    void *oi) {
    const int64_t per = vec ? 16 / (int64_t)sizeof(T) : 1;
    ArgFlatArgs a;
    a.nd = nd;
    a.is_max = is_max;
    a.skipna = skipna;
    a.idx0 = idx0;
    a.tail0 = a.tailn = 0;
    for (int d = 0; d < 4; ++d) {
        const int s = d - (4 - nd);
        a.shp[d] = s >= 0 ? shape[s] : 1;
        a.str[d] = s >= 0 ? strides[s] : 0;
        a.mult[d] = s >= 0 ? mult[s] : 0;
        if (vec && d < 3) a.str[d] /= per;
    }
    if (vec) {
        a.tail0 = (a.shp[3] / per) * per;
        a.tailn = a.shp[3] - a.tail0;     // nonzero only when nd == 1
        a.shp[3] /= per;
        a.nunits = n / shape[nd - 1] * a.shp[3];
    } else {
        a.nunits = n;
    }
    int64_t blocks = (a.nunits + 255) / 256;
    if (blocks > ARG_GRID_CAP) blocks = ARG_GRID_CAP;
    if (blocks < 1) blocks = 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const T *src = static_cast<const T *>(in) + in_off;
    if (vec)
        hipLaunchKernelGGL((arg_flat_s1<T, uint4>), dim3((unsigned)blocks),
                           dim3(256), 0, st, src, a, static_cast<T *>(sv),
                           static_cast<int64_t *>(si));
    else
        hipLaunchKernelGGL((arg_flat_s1<T, T>), dim3((unsigned)blocks),
                           dim3(256), 0, st, src, a, static_cast<T *>(sv),
                           static_cast<int64_t *>(si));
    if (launched("rt_arg_flat(1)")) return 1;
    hipLaunchKernelGGL((arg_flat_s2<T>), dim3(1), dim3(256), 0, st,
                       static_cast<const T *>(sv),
                       static_cast<const int64_t *>(si), (int)blocks,
                       static_cast<T *>(ov), static_cast<int64_t *>(oi),
                       is_max, skipna);
    return launched("rt_arg_flat(2)");
}

// -- one axis ----------------------------------------------------------------

struct ArgAxisArgs {
    int64_t nout;
    int64_t oshp[3], ostr[3];   // kept axes, right-aligned: extent, in-stride
    int64_t K, kstr, idx0;      // reduced axis
    int64_t C, clen;            // chunks of the reduced axis (thread regime)
    int is_max, skipna;
};

__device__ __forceinline__ int64_t arg_line_off(const ArgAxisArgs &a,
                                                int64_t o) {
    uint64_t rem = (uint64_t)o;
    int64_t off = 0;
#pragma unroll
    for (int d = 2; d >= 0; --d) {
        const uint64_t q = rem / (uint64_t)a.oshp[d];
        off += (int64_t)(rem - q * (uint64_t)a.oshp[d]) * a.ostr[d];
        rem = q;
    }
    return off;
}

// reduced axis innermost: one wave per line, lanes stride the line in load
// units, four loads in flight per lane.  L = uint4 (the host checked: axis
// stride 1, every line 16-byte aligned) leaves the K % PER last elements
// to a scalar tail.
template <typename T, typename L, int MX, int SK>
__device__ __forceinline__ void arg_line_walk(const T *__restrict__ line,
                                              const ArgAxisArgs &a, int lane,
                                              T &bv, int64_t &bi) {
    constexpr int PER = sizeof(L) / sizeof(T);
    const L *src = reinterpret_cast<const L *>(line);
    const int64_t units = a.K / PER;
    const int64_t us = PER > 1 ? 1 : a.kstr;
    int64_t u = lane;
    for (; u + 192 < units; u += 256) {
        const L x0 = src[u * us];
        const L x1 = src[(u + 64) * us];
        const L x2 = src[(u + 128) * us];
        const L x3 = src[(u + 192) * us];
        arg_unit_acc<T, L, MX, SK>(x0, a.idx0 + u * PER, 1, bv, bi);
        arg_unit_acc<T, L, MX, SK>(x1, a.idx0 + (u + 64) * PER, 1, bv, bi);
        arg_unit_acc<T, L, MX, SK>(x2, a.idx0 + (u + 128) * PER, 1, bv, bi);
        arg_unit_acc<T, L, MX, SK>(x3, a.idx0 + (u + 192) * PER, 1, bv, bi);
    }
    for (; u < units; u += 64) {
        const L x0 = src[u * us];
        arg_unit_acc<T, L, MX, SK>(x0, a.idx0 + u * PER, 1, bv, bi);
    }
    if (PER > 1) {
        const int64_t k = units * PER + lane;
        if (k < a.K)
            arg_unit_acc<T, T, MX, SK>(line[k], a.idx0 + k, 1, bv, bi);
    }
}

// one chunk [k, k1) of one line, by one thread
template <typename T, int MX, int SK>
__device__ __forceinline__ void arg_chunk_walk(const T *__restrict__ line,
                                               const ArgAxisArgs &a,
                                               int64_t k, int64_t k1, T &bv,
                                               int64_t &bi) {
    for (; k + 3 < k1; k += 4) {            // four loads in flight
        const T v0 = line[k * a.kstr];
        const T v1 = line[(k + 1) * a.kstr];
        const T v2 = line[(k + 2) * a.kstr];
        const T v3 = line[(k + 3) * a.kstr];
        arg_unit_acc<T, T, MX, SK>(v0, a.idx0 + k, 1, bv, bi);
        arg_unit_acc<T, T, MX, SK>(v1, a.idx0 + k + 1, 1, bv, bi);
        arg_unit_acc<T, T, MX, SK>(v2, a.idx0 + k + 2, 1, bv, bi);
        arg_unit_acc<T, T, MX, SK>(v3, a.idx0 + k + 3, 1, bv, bi);
    }
    for (; k < k1; ++k)
        arg_unit_acc<T, T, MX, SK>(line[k * a.kstr], a.idx0 + k, 1, bv, bi);
}

template <typename T, typename L>
__global__ __launch_bounds__(256) void arg_axis_wave(
    const T *__restrict__ in, ArgAxisArgs a, T *__restrict__ ov,
    int64_t *__restrict__ oi) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
         o < a.nout; o += nwaves) {
        const T *line = in + arg_line_off(a, o);
        T bv = T(0);
        int64_t bi = -1;
#define BODY(MX, SK) arg_line_walk<T, L, MX, SK>(line, a, lane, bv, bi)
        ARG_FLAGS(a.is_max, a.skipna, BODY);
#undef BODY
        arg_wave_reduce<T>(bv, bi, a.is_max, a.skipna);
        if (lane == 0) {
            ov[o] = bv;
            oi[o] = bi;
        }
    }
}

// reduced axis not innermost: one thread per (chunk, output element),
// consecutive threads on consecutive outputs (coalesced); pair t goes to
// ov/oi[t], t = chunk * nout + output.  C == 1 is the plain regime.
template <typename T>
__global__ __launch_bounds__(256) void arg_axis_thread(
    const T *__restrict__ in, ArgAxisArgs a, T *__restrict__ ov,
    int64_t *__restrict__ oi) {
    const int64_t total = a.nout * a.C;
    const int64_t S = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total;
         t += S) {
        const int64_t c = t / a.nout, o = t - c * a.nout;
        const int64_t off = arg_line_off(a, o);
        int64_t k1 = (c + 1) * a.clen;
        if (k1 > a.K) k1 = a.K;
        T bv = T(0);
        int64_t bi = -1;
#define BODY(MX, SK)                                                       \
    arg_chunk_walk<T, MX, SK>(in + off, a, c * a.clen, k1, bv, bi)
        ARG_FLAGS(a.is_max, a.skipna, BODY);
#undef BODY
        ov[t] = bv;
        oi[t] = bi;
    }
}

// the chunks' pairs (C, nout) -> one pair per output element
template <typename T>
__global__ __launch_bounds__(256) void arg_pairs_reduce(
    const T *__restrict__ pv, const int64_t *__restrict__ pi, int64_t C,
    int64_t nout, T *__restrict__ ov, int64_t *__restrict__ oi, int mx,
    int sk) {
    const int64_t S = (int64_t)gridDim.x * 256;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < nout;
         o += S) {
        T bv = T(0);
        int64_t bi = -1;
        for (int64_t c = 0; c < C; ++c)
            arg_take<T>(bv, bi, pv[c * nout + o], pi[c * nout + o], mx, sk);
        ov[o] = bv;
        oi[o] = bi;
    }
}

unsigned arg_blocks(int64_t threads) {
    int64_t b = (threads + 255) / 256;
    if (b > 4096) b = 4096;
    if (b < 1) b = 1;
    return (unsigned)b;
}

template <typename T>
int arg_axis_launch(uintptr_t stream, const void *in, int64_t in_off,
                    const ArgAxisArgs &a, bool wave, bool vec, void *pv,
                    void *pi, void *ov, void *oi) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const T *src = static_cast<const T *>(in) + in_off;
    T *outv = static_cast<T *>(ov);
    int64_t *outi = static_cast<int64_t *>(oi);
    if (wave) {
        if (vec)
            hipLaunchKernelGGL((arg_axis_wave<T, uint4>),
                               dim3(arg_blocks(a.nout * 64)), dim3(256), 0,
                               st, src, a, outv, outi);
        else
            hipLaunchKernelGGL((arg_axis_wave<T, T>),
                               dim3(arg_blocks(a.nout * 64)), dim3(256), 0,
                               st, src, a, outv, outi);
        return launched("rt_arg_axis(wave)");
    }
    if (a.C == 1) {
        hipLaunchKernelGGL((arg_axis_thread<T>), dim3(arg_blocks(a.nout)),
                           dim3(256), 0, st, src, a, outv, outi);
        return launched("rt_arg_axis(thread)");
    }
    hipLaunchKernelGGL((arg_axis_thread<T>), dim3(arg_blocks(a.nout * a.C)),
                       dim3(256), 0, st, src, a, static_cast<T *>(pv),
                       static_cast<int64_t *>(pi));
    if (launched("rt_arg_axis(chunks)")) return 1;
    hipLaunchKernelGGL((arg_pairs_reduce<T>), dim3(arg_blocks(a.nout)),
                       dim3(256), 0, st, static_cast<const T *>(pv),
                       static_cast<const int64_t *>(pi), a.C, a.nout, outv,
                       outi, a.is_max, a.skipna);
    return launched("rt_arg_axis(pairs)");
}

// -- pair combine (rt_combine_box for pairs) ----------------------------------

struct ArgBoxArgs {
    int64_t n;
    int64_t shape[4], dvs[4], dis[4], ss[4];
    int nd, is_max, skipna;
};

template <typename T>
__global__ __launch_bounds__(256) void arg_combine_kernel(
    T *__restrict__ dv, int64_t *__restrict__ di, const T *__restrict__ sv,
    const int64_t *__restrict__ si, ArgBoxArgs a) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < a.n; i += stride) {
        int64_t rem = i, so = 0, vo = 0, io = 0;
        for (int d = a.nd - 1; d >= 0; --d) {
            const int64_t idx = rem % a.shape[d];
            rem /= a.shape[d];
            so += idx * a.ss[d];
            vo += idx * a.dvs[d];
            io += idx * a.dis[d];
        }
        const T v = sv[so];
        const int64_t k = si[so];
        if (rt_arg_better<T>(v, k, dv[vo], di[io], a.is_max, a.skipna)) {
            dv[vo] = v;
            di[io] = k;
        }
    }
}

template <typename T>
int arg_combine_launch(uintptr_t stream, void *dv, void *di, const void *sv,
                       const void *si, int64_t dv_off, int64_t di_off,
                       const ArgBoxArgs &a) {
    int64_t blocks = (a.n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL((arg_combine_kernel<T>), dim3((unsigned)blocks),
                       dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       static_cast<T *>(dv) + dv_off,
                       static_cast<int64_t *>(di) + di_off,
                       static_cast<const T *>(sv),
                       static_cast<const int64_t *>(si), a);
    return launched("rt_arg_combine_box");
}

}  // namespace

extern "C" int rt_arg_grid_cap(void) { return ARG_GRID_CAP; }

extern "C" int rt_arg_flat_regime(const void *in, int64_t in_off, int nd,
                                  const int64_t *shape,
                                  const int64_t *strides, int dtype) {
    int64_t n;
    if (arg_validate("rt_arg_flat_regime", in, nd, shape, strides, dtype, &n))
        return -1;
    return arg_flat_vec(in, in_off, nd, shape, strides, dtype_size(dtype))
               ? 1 : 0;
}

extern "C" int rt_arg_flat(uintptr_t stream, const void *in, int64_t in_off,
                           int nd, const int64_t *shape,
                           const int64_t *strides, const int64_t *mult,
                           int64_t idx0, int dtype, int is_max, int skipna,
                           void *scratch_vals, void *scratch_idx,
                           void *out_val, void *out_idx) {
    int64_t n;
    if (arg_validate("rt_arg_flat", in, nd, shape, strides, dtype, &n))
        return 1;
    if (!mult || !scratch_vals || !scratch_idx || !out_val || !out_idx) {
        set_error("rt_arg_flat: NULL argument");
        return 1;
    }
    return dtype_dispatch<7>("rt_arg_flat", dtype, [&](auto t) {
        using T = decltype(t);
        const bool vec =
            arg_flat_vec(in, in_off, nd, shape, strides, sizeof(T));
        return arg_flat_launch<T>(stream, in, in_off, nd, shape, strides,
                                  mult, idx0, n, vec, is_max != 0,
                                  skipna != 0, scratch_vals, scratch_idx,
                                  out_val, out_idx);
    });
}

extern "C" int rt_arg_axis(uintptr_t stream, const void *in, int64_t in_off,
                           int nd, const int64_t *shape,
                           const int64_t *strides, int axis, int64_t idx0,
                           int dtype, int is_max, int skipna,
                           int64_t nchunks, void *part_vals, void *part_idx,
                           void *out_vals, void *out_idx) {
    int64_t n;
    if (arg_validate("rt_arg_axis", in, nd, shape, strides, dtype, &n))
        return 1;
    if (axis < 0 || axis >= nd) {
        set_error("rt_arg_axis: axis out of range");
        return 1;
    }
    if (!out_vals || !out_idx) {
        set_error("rt_arg_axis: NULL output");
        return 1;
    }
    const bool wave = axis == nd - 1;
    if (nchunks < 1 || nchunks > shape[axis]
        || (nchunks > 1 && (wave || !part_vals || !part_idx))) {
        set_error("rt_arg_axis: bad chunking");
        return 1;
    }
    ArgAxisArgs a;
    a.K = shape[axis];
    a.kstr = strides[axis];
    a.idx0 = idx0;
    a.C = nchunks;
    a.clen = (a.K + nchunks - 1) / nchunks;
    a.is_max = is_max != 0;
    a.skipna = skipna != 0;
    a.nout = n / a.K;
    for (int d = 0; d < 3; ++d) {
        a.oshp[d] = 1;
        a.ostr[d] = 0;
    }
    int slot = 2;
    for (int d = nd - 1; d >= 0; --d) {
        if (d == axis) continue;
        a.oshp[slot] = shape[d];
        a.ostr[slot] = strides[d];
        --slot;
    }
    // wave regime with 16-byte loads: axis stride 1 and every line start
    // (base + any combination of kept-axis strides) 16-byte aligned
    return dtype_dispatch<7>("rt_arg_axis", dtype, [&](auto t) {
        using T = decltype(t);
        const int es = sizeof(T);
        bool vec = wave && strides[axis] == 1 && shape[axis] >= 16 / es
            && (reinterpret_cast<uintptr_t>(in) + (uint64_t)(in_off * es))
                   % 16 == 0;
        for (int d = 0; vec && d < nd - 1; ++d)
            vec = (strides[d] * es) % 16 == 0;
        return arg_axis_launch<T>(stream, in, in_off, a, wave, vec,
                                  part_vals, part_idx, out_vals, out_idx);
    });
}

extern "C" int rt_arg_combine_box(uintptr_t stream, void *dst_vals,
                                  void *dst_idx, const void *src_vals,
                                  const void *src_idx, int nd,
                                  const int64_t *shape,
                                  const int64_t *dst_val_strides,
                                  const int64_t *dst_idx_strides,
                                  const int64_t *src_strides,
                                  int64_t dst_val_off, int64_t dst_idx_off,
                                  int dtype, int is_max, int skipna) {
    int64_t n;
    if (arg_validate("rt_arg_combine_box", src_vals, nd, shape, src_strides,
                     dtype, &n))
        return 1;
    if (!dst_vals || !dst_idx || !src_idx || !dst_val_strides
        || !dst_idx_strides) {
        set_error("rt_arg_combine_box: NULL argument");
        return 1;
    }
    ArgBoxArgs a;
    a.nd = nd;
    a.n = n;
    a.is_max = is_max != 0;
    a.skipna = skipna != 0;
    for (int d = 0; d < 4; ++d) {
        a.shape[d] = d < nd ? shape[d] : 1;
        a.dvs[d] = d < nd ? dst_val_strides[d] : 0;
        a.dis[d] = d < nd ? dst_idx_strides[d] : 0;
        a.ss[d] = d < nd ? src_strides[d] : 0;
    }
    return dtype_dispatch<7>("rt_arg_combine_box", dtype, [&](auto t) {
        return arg_combine_launch<decltype(t)>(stream, dst_vals, dst_idx,
                                               src_vals, src_idx,
                                               dst_val_off, dst_idx_off, a);
    });
}

// ---------------------------------------------------------------------------
// Dense GEMM on the matrix units: C[M,N] (+)= A[M,K] @ B[K,N], float32 and
// float64 (the local np.dot of the reference's matmul workers,
// ramba/ramba.py:3056, :6953-7040).
//
// One block of 256 lanes (4 waves, 2 x 2) owns a 128 x 128 tile of C and walks
// K in steps of BK (64 bytes of an A row: 16 floats / 8 doubles).  Each wave
// keeps its 64 x 64 sub-tile in accumulator registers: 2 x 2 tiles of
// v_mfma_f32_32x32x2 or 4 x 4 tiles of v_mfma_f64_16x16x4.  The A and B
// panels of a step go global -> registers -> LDS, LDS double-buffered; the
// global loads of step k+1 are issued before the MFMAs of step k and stored
// to the other buffer after them, one barrier per step.
//
// LDS holds both panels k-major: As[k][m] and Bs[k][n], so the MFMA operand
// of lane l (A[l % T][l / T], B[l / T][l % T], T = 32 or 16) is a read of T
// consecutive elements per k row.  Row strides are padded (GemmT::LDA/LDB)
// by bank arithmetic (64 four-byte banks, 32 lanes per pass assumed; not
// measured): fp64 rows are 16 doubles apart modulo 32, so the two k rows a
// half-wave reads fall on disjoint banks; the fp32 A stride of 130 spreads
// the transposing stores of the 16-byte path to a two-way collision.
//
// Two global-load paths per operand, picked on the host (gemm_paths):
//   16-byte : A with a_cs == 1 (a chunk runs along k and is scattered down
//             an LDS column), B with b_cs == 1 (a chunk runs along n and is
//             stored whole); base and row stride 16-byte aligned.  A chunk
//             that straddles the edge falls back to element loads.
//   element : any strides; lanes run along m (A) / n (B).
// Rows, columns and k outside the problem are never read and enter LDS as
// zeros, on BOTH operands in the K tail (0 x inf from a real element would
// otherwise reach a real output); outside rows and columns are never stored.
// Every output element is summed by one wave in ascending k: no atomics, no
// split-K, bit-reproducible.
//
// A batch of products (rt_gemm_batched) is the same kernel over batch x tiles
// tile indices, batch-major: tile index / tiles is the batch entry, whose
// a_bs / b_bs / c_bs element offsets move the three base pointers (0: the
// operand is shared by every entry).  rt_gemm is the batch == 1 call.
// ---------------------------------------------------------------------------

namespace {

enum { GEMM_BM = 128, GEMM_BN = 128, GEMM_GRID_CAP = 1 << 20 };

template <typename T>
struct GemmT;

template <>
struct GemmT<float> {
    // 32x32x2: lane l gives A[l%32][l/32], B[l/32][l%32]; holds 16 of D
    enum { BK = 16, VEC = 4, TM = 32, KM = 2, RPT = 16, LDA = 130, LDB = 132 };
    typedef float acc_t __attribute__((ext_vector_type(16)));
    typedef float vec_t __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
    }
    // row of D held in register r by a lane of k group lk = l / 32
    static __device__ __forceinline__ int row(int r, int lk) {
        return 8 * (r / 4) + 4 * lk + r % 4;
    }
};

template <>
struct GemmT<double> {
    // 16x16x4: lane l gives A[l%16][l/16], B[l/16][l%16]; holds 4 of D
    enum { BK = 8, VEC = 2, TM = 16, KM = 4, RPT = 4, LDA = 144, LDB = 144 };
    typedef double acc_t __attribute__((ext_vector_type(4)));
    typedef double vec_t __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ acc_t mfma(double a, double b, acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    // row of D held in register r by a lane of k group lk = l / 16: the
    // four registers interleave the lane groups (pinned by the exact test)
    static __device__ __forceinline__ int row(int r, int lk) {
        return 4 * r + lk;
    }
};

struct GemmArgs {
    int64_t M, N, K;
    int64_t a_rs, a_cs, b_rs, b_cs, ldc;
    int64_t a_bs, b_bs, c_bs;       // batch strides (elements)
    int64_t batch, ntiles;          // ntiles = batch * tiles of one entry
    int accumulate;
};

// One 16-byte chunk of VEC elements at p, of which `valid` (<= 0: none) lie
// inside the problem; a partial chunk is read element by element.
template <typename T>
__device__ __forceinline__ typename GemmT<T>::vec_t gemm_chunk(
    const T *p, int64_t valid) {
    typedef typename GemmT<T>::vec_t vec_t;
    constexpr int VEC = GemmT<T>::VEC;
    vec_t v = {};
    if (valid >= VEC) {
        v = *reinterpret_cast<const vec_t *>(p);
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            if (i < valid) v[i] = p[i];
    }
    return v;
}

// Global -> registers for one k step of one operand.  r holds the thread's
// EPT = 128 * BK / 256 elements of the 128 x BK panel.
//   KVEC  (A, a_cs == 1): chunk c = t + 256 j covers row c / 4, k (c % 4) VEC..
//   MNVEC (B, b_cs == 1): chunk c covers k c / CPR, columns (c % CPR) VEC..
//   ELEM: element e = t + 256 j is (mn e % 128, k e / 128).
// mn0 / MN: tile origin and extent along m (A) or n (B); mn_s / k_s strides.
enum { GEMM_ELEM = 0, GEMM_KVEC = 1, GEMM_MNVEC = 2 };

template <typename T, int PATH>
__device__ __forceinline__ void gemm_load(
    const T *__restrict__ p, int64_t mn_s, int64_t k_s, int64_t mn0,
    int64_t MN, int64_t k0, int64_t K, int t,
    T (&r)[GEMM_BM * GemmT<T>::BK / 256]) {
    typedef GemmT<T> G;
    constexpr int VEC = G::VEC, EPT = GEMM_BM * G::BK / 256;
    static_assert(G::BK / VEC == 4, "4 chunks (64 bytes) per panel row");
    if constexpr (PATH == GEMM_KVEC) {
#pragma unroll
        for (int j = 0; j < EPT / VEC; ++j) {
            const int c = t + 256 * j;
            const int64_t mn = mn0 + (c >> 2), k = k0 + (c & 3) * VEC;
            typename G::vec_t v = {};
            if (mn < MN) v = gemm_chunk<T>(p + mn * mn_s + k, K - k);
#pragma unroll
            for (int i = 0; i < VEC; ++i) r[j * VEC + i] = v[i];
        }
    } else if constexpr (PATH == GEMM_MNVEC) {
        constexpr int CPR = GEMM_BN / VEC;
#pragma unroll
        for (int j = 0; j < EPT / VEC; ++j) {
            const int c = t + 256 * j;
            const int64_t k = k0 + c / CPR, mn = mn0 + (c % CPR) * VEC;
            typename G::vec_t v = {};
            if (k < K) v = gemm_chunk<T>(p + k * k_s + mn, MN - mn);
#pragma unroll
            for (int i = 0; i < VEC; ++i) r[j * VEC + i] = v[i];
        }
    } else {
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int e = t + 256 * j;
            const int64_t mn = mn0 + (e & 127), k = k0 + (e >> 7);
            r[j] = (mn < MN && k < K) ? p[mn * mn_s + k * k_s] : T(0);
        }
    }
}

// Registers -> the k-major LDS panel s[k * LD + mn], same element mapping.
template <typename T, int PATH, int LD>
__device__ __forceinline__ void gemm_stage(
    T *s, int t, const T (&r)[GEMM_BM * GemmT<T>::BK / 256]) {
    typedef GemmT<T> G;
    constexpr int VEC = G::VEC, EPT = GEMM_BM * G::BK / 256;
    if constexpr (PATH == GEMM_KVEC) {
#pragma unroll
        for (int j = 0; j < EPT / VEC; ++j) {
            const int c = t + 256 * j;
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                s[((c & 3) * VEC + i) * LD + (c >> 2)] = r[j * VEC + i];
        }
    } else if constexpr (PATH == GEMM_MNVEC) {
        constexpr int CPR = GEMM_BN / VEC;
        static_assert((LD * sizeof(T)) % 16 == 0, "16-byte LDS rows");
#pragma unroll
        for (int j = 0; j < EPT / VEC; ++j) {
            const int c = t + 256 * j;
            typename G::vec_t v;
#pragma unroll
            for (int i = 0; i < VEC; ++i) v[i] = r[j * VEC + i];
            *reinterpret_cast<typename G::vec_t *>(
                &s[(c / CPR) * LD + (c % CPR) * VEC]) = v;
        }
    } else {
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int e = t + 256 * j;
            s[(e >> 7) * LD + (e & 127)] = r[j];
        }
    }
}

// The kernel is compiled with the packed-fp32 VALU forms (v_pk_*_f32) off:
// its only VALU float math is the accumulate epilogue `C + acc`, which is to
// stay one IEEE add per element whatever the compiler's vectoriser prefers.
// The attribute covers this function and what is inlined into it only (the
// host pass does not know the feature, so it sees nothing).
#if defined(__HIP_DEVICE_COMPILE__)
#define GEMM_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define GEMM_NO_PK_F32
#endif

// A block-uniform 64-bit value, held in scalar registers.
__device__ __forceinline__ int64_t gemm_uniform(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

template <typename T, int PA, int PB>
__global__ __launch_bounds__(256) GEMM_NO_PK_F32 void gemm_kernel(
    T *__restrict__ c0, const T *__restrict__ a0, const T *__restrict__ b0,
    GemmArgs g) {
    typedef GemmT<T> G;
    constexpr int BK = G::BK, TM = G::TM, KM = G::KM, NT = 64 / TM;
    constexpr int EPT = GEMM_BM * BK / 256;
    static_assert(GEMM_BM == 128 && GEMM_BN == 128, "2 x 2 waves of 64 x 64");
    __shared__ __attribute__((aligned(16))) T As[2][BK * G::LDA];
    __shared__ __attribute__((aligned(16))) T Bs[2][BK * G::LDB];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int lr = lane % TM, lk = lane / TM;
    const int64_t nk = (g.K + BK - 1) / BK;
    const int64_t tiles_n = (g.N + GEMM_BN - 1) / GEMM_BN;
    const int64_t tiles = (g.M + GEMM_BM - 1) / GEMM_BM * tiles_n;

    for (int64_t tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
        // (block-uniform, but the 64-bit division runs on the vector unit:
        // moved to scalar registers so the offsets below cost no VGPRs)
        const int64_t bi = gemm_uniform(tile / tiles);
        const int64_t bt = gemm_uniform(tile % tiles);
        const int64_t m0 = (bt / tiles_n) * GEMM_BM;
        const int64_t n0 = (bt % tiles_n) * GEMM_BN;
        const T *__restrict__ a = a0 + bi * g.a_bs;
        const T *__restrict__ b = b0 + bi * g.b_bs;
        T *__restrict__ c = c0 + bi * g.c_bs;
        typename G::acc_t acc[NT][NT];
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = {};
        T ra[EPT], rb[EPT];

        gemm_load<T, PA>(a, g.a_rs, g.a_cs, m0, g.M, 0, g.K, t, ra);
        gemm_load<T, PB>(b, g.b_cs, g.b_rs, n0, g.N, 0, g.K, t, rb);
        gemm_stage<T, PA, G::LDA>(As[0], t, ra);
        gemm_stage<T, PB, G::LDB>(Bs[0], t, rb);
        __syncthreads();

        int cur = 0;
        for (int64_t kt = 0; kt < nk; ++kt) {
            const bool more = kt + 1 < nk;
            if (more) {
                const int64_t k0 = (kt + 1) * BK;
                gemm_load<T, PA>(a, g.a_rs, g.a_cs, m0, g.M, k0, g.K, t, ra);
                gemm_load<T, PB>(b, g.b_cs, g.b_rs, n0, g.N, k0, g.K, t, rb);
            }
            const T *Ac = As[cur], *Bc = Bs[cur];
#pragma unroll
            for (int kk = 0; kk < BK; kk += KM) {
                T af[NT], bf[NT];
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    af[i] = Ac[(kk + lk) * G::LDA + wm + i * TM + lr];
                    bf[i] = Bc[(kk + lk) * G::LDB + wn + i * TM + lr];
                }
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        acc[i][j] = G::mfma(af[i], bf[j], acc[i][j]);
            }
            if (more) {
                gemm_stage<T, PA, G::LDA>(As[cur ^ 1], t, ra);
                gemm_stage<T, PB, G::LDB>(Bs[cur ^ 1], t, rb);
            }
            // the next step reads what was just staged, and the step after
            // it overwrites the buffer read above
            __syncthreads();
            cur ^= 1;
        }

        // register r of a tile is row G::row(r, lane / T), column lane % T
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < G::RPT; ++r) {
                    const int64_t row = m0 + wm + i * TM + G::row(r, lk);
                    const int64_t col = n0 + wn + j * TM + lr;
                    if (row < g.M && col < g.N) {
                        T *p = c + row * g.ldc + col;
                        T v = acc[i][j][r];
                        if (g.accumulate) v = *p + v;
                        *p = v;
                    }
                }
    }
}

// Which load path each operand takes: 16-byte when its unit stride runs
// along the panel's fast axis and base, row stride and (with more than one
// batch entry) batch stride are 16-byte aligned.
template <typename T>
void gemm_paths(const void *a, const void *b, const GemmArgs &g, bool *va,
                bool *vb) {
    const int64_t per = 16 / (int64_t)sizeof(T);
    const bool many = g.batch > 1;
    *va = g.a_cs == 1 && g.a_rs % per == 0 && !(many && g.a_bs % per)
          && reinterpret_cast<uintptr_t>(a) % 16 == 0;
    *vb = g.b_cs == 1 && g.b_rs % per == 0 && !(many && g.b_bs % per)
          && reinterpret_cast<uintptr_t>(b) % 16 == 0;
}

template <typename T>
int gemm_launch(uintptr_t stream, void *c, const void *a, const void *b,
                const GemmArgs &g) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    bool va, vb;
    gemm_paths<T>(a, b, g, &va, &vb);
    const unsigned blocks = (unsigned)(g.ntiles < GEMM_GRID_CAP
                                           ? g.ntiles : GEMM_GRID_CAP);
#define GEMM_GO(PA, PB)                                                    \
    hipLaunchKernelGGL((gemm_kernel<T, PA, PB>), dim3(blocks), dim3(256),  \
                       0, st, static_cast<T *>(c),                         \
                       static_cast<const T *>(a),                          \
                       static_cast<const T *>(b), g)
    if (va && vb) GEMM_GO(GEMM_KVEC, GEMM_MNVEC);
    else if (va) GEMM_GO(GEMM_KVEC, GEMM_ELEM);
    else if (vb) GEMM_GO(GEMM_ELEM, GEMM_MNVEC);
    else GEMM_GO(GEMM_ELEM, GEMM_ELEM);
#undef GEMM_GO
    return launched("gemm");
}

// Validation and launch behind rt_gemm (batch 1) and rt_gemm_batched.
int gemm_run(const char *who, uintptr_t stream, void *c, const void *a,
             const void *b, int64_t batch, int64_t M, int64_t N, int64_t K,
             int64_t a_rs, int64_t a_cs, int64_t b_rs, int64_t b_cs,
             int64_t ldc, int64_t a_bs, int64_t b_bs, int64_t c_bs, int dtype,
             int accumulate) {
    if (dtype != RT_F64 && dtype != RT_F32) return fail(who, "bad dtype");
    if (accumulate != 0 && accumulate != 1)
        return fail(who, "bad accumulate");
    if (batch < 0) return fail(who, "negative batch");
    if (M < 0 || N < 0 || K < 0) return fail(who, "negative extent (M/N/K)");
    const int64_t lim = 1LL << 40, plim = 1LL << 46;
    if (batch >= lim) return fail(who, "batch out of range");
    if (M >= lim || N >= lim || K >= lim)
        return fail(who, "extent out of range (M/N/K)");
    if ((N && M > plim / N) || (K && M > plim / K) || (N && K > plim / N))
        return fail(who, "shape too large (M*N, M*K or K*N)");
    // (each product is at most 2^46 here, so the divisions are exact enough)
    if (batch && ((M * N && batch > plim / (M * N))
                  || (M * K && batch > plim / (M * K))
                  || (K * N && batch > plim / (K * N))))
        return fail(who, "batch too large (batch*M*N, batch*M*K or "
                         "batch*K*N)");
    if (ldc < N) return fail(who, "ldc < N");
    if (batch > 1 && M && N && c_bs < (M - 1) * ldc + N)
        return fail(who, "c_bs < (M-1)*ldc + N");
    if (batch == 0 || M == 0 || N == 0) return 0;
    if (!c) return fail(who, "NULL c");
    if (K && (!a || !b)) return fail(who, "NULL a/b");
    if (K == 0 && accumulate) return 0;
    GemmArgs g;
    g.M = M, g.N = N, g.K = K;
    g.a_rs = a_rs, g.a_cs = a_cs, g.b_rs = b_rs, g.b_cs = b_cs, g.ldc = ldc;
    g.a_bs = a_bs, g.b_bs = b_bs, g.c_bs = c_bs;
    g.batch = batch;
    g.ntiles = batch * ((M + GEMM_BM - 1) / GEMM_BM)
               * ((N + GEMM_BN - 1) / GEMM_BN);
    g.accumulate = accumulate;
    if (dtype == RT_F64) return gemm_launch<double>(stream, c, a, b, g);
    return gemm_launch<float>(stream, c, a, b, g);
}

}  // namespace

extern "C" int rt_gemm_tile(int dtype, int *bm, int *bn, int *bk) {
    const char *who = "rt_gemm_tile";
    if (dtype != RT_F64 && dtype != RT_F32) return fail(who, "bad dtype");
    if (!bm || !bn || !bk) return fail(who, "NULL output");
    *bm = GEMM_BM;
    *bn = GEMM_BN;
    *bk = dtype == RT_F64 ? (int)GemmT<double>::BK : (int)GemmT<float>::BK;
    return 0;
}

extern "C" int rt_gemm_batched(uintptr_t stream, void *c, const void *a,
                               const void *b, int64_t batch, int64_t M,
                               int64_t N, int64_t K, int64_t a_rs,
                               int64_t a_cs, int64_t b_rs, int64_t b_cs,
                               int64_t ldc, int64_t a_bs, int64_t b_bs,
                               int64_t c_bs, int dtype, int accumulate) {
    return gemm_run("rt_gemm_batched", stream, c, a, b, batch, M, N, K, a_rs,
                    a_cs, b_rs, b_cs, ldc, a_bs, b_bs, c_bs, dtype,
                    accumulate);
}

extern "C" int rt_gemm(uintptr_t stream, void *c, const void *a,
                       const void *b, int64_t M, int64_t N, int64_t K,
                       int64_t a_rs, int64_t a_cs, int64_t b_rs,
                       int64_t b_cs, int64_t ldc, int dtype,
                       int accumulate) {
    return gemm_run("rt_gemm", stream, c, a, b, 1, M, N, K, a_rs, a_cs, b_rs,
                    b_cs, ldc, 0, 0, 0, dtype, accumulate);
}


// ---------------------------------------------------------------------------
// Matrix-vector product: y[M] (+)= A[M,K] @ x[K], float32 and float64; x @ A
// is the same call on A's transposed strides.  The kernels are bound by
// reading A once, so each orientation gets lanes running along A's unit
// stride (regimes, picked on the host by gemv_regime):
//
//   ROW_VEC / ROW_ELEM (a_cs == 1, the reduction runs along the unit stride):
//     a block of 4 waves owns GEMV_ROW_R = 16 rows, one wave per 4 rows.  The
//     block stages GEMV_ROW_S = 1024 elements of x in LDS once per k step;
//     the wave's lanes walk the step 16 bytes at a time (ROW_VEC: base and
//     row stride 16-byte aligned) or one element at a time (ROW_ELEM), each
//     lane loading from its 4 rows before it multiplies, and keep 4 private
//     sums.  A fixed shuffle tree (offsets 32 .. 1) finishes each row.
//   COL_VEC / COL_ELEM (lanes along m; the reduction runs across rows of
//     memory): a block owns GEMV_COL_R = 256 outputs and stages GEMV_COL_S =
//     256 elements of x per step.  COL_VEC (a_rs == 1, base and a_cs 16-byte
//     aligned): a thread owns VEC consecutive outputs (one 16-byte load per
//     k), so 256 / VEC threads cover the outputs and the VEC thread groups
//     interleave over k; group 0 adds the other groups' sums from LDS in
//     ascending group order.  COL_ELEM: one output per thread, any strides
//     (the untuned general case, and a_rs == 1 without alignment).
//
// K-split: blockIdx.y = range r covers k in [r klen, (r + 1) klen), klen =
// ceil(K / ksplit) rounded up to the k step; only the ceil(K / klen)
// non-empty ranges are launched.  With ksplit > 1 a block writes its sums to
// scratch[r M + m] and gemv_finish_kernel adds the ranges in ascending order
// (and applies accumulate).  No atomics anywhere: (shape, strides, ksplit)
// fixes the summation order, hence the bits.  Lanes past the end of a row, a
// k range or M skip the multiply, so no fill value ever meets an operand.
// ---------------------------------------------------------------------------

namespace {

enum { GEMV_ROW_R = 16, GEMV_ROW_S = 1024, GEMV_COL_R = 256, GEMV_COL_S = 256,
       GEMV_MAX_SPLIT = 4096, GEMV_GRID_CAP = 1 << 20 };
enum { GEMV_ROW_VEC = 0, GEMV_ROW_ELEM = 1, GEMV_COL_VEC = 2,
       GEMV_COL_ELEM = 3 };

struct GemvArgs {
    int64_t M, K, a_rs, a_cs, x_s, y_s;
    int64_t klen;           // k per blockIdx.y, a multiple of the k step
    int accumulate, split;  // split: sums go to part[blockIdx.y * M + m]
};

// VEC elements at p: one 16-byte load (VEC > 1) or one element.
template <typename T, int VEC>
__device__ __forceinline__ void gemv_ld(const T *p, T (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = *p;
    } else {
        typedef T vec_t __attribute__((ext_vector_type(VEC)));
        const vec_t w = *reinterpret_cast<const vec_t *>(p);
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = w[i];
    }
}

template <typename T>
__device__ __forceinline__ void gemv_store(T *y, T *part, const GemvArgs &g,
                                           int64_t m, T v) {
    if (g.split) {
        part[(int64_t)blockIdx.y * g.M + m] = v;
    } else {
        T *p = y + m * g.y_s;
        *p = g.accumulate ? *p + v : v;
    }
}

// One k step of one wave of the row kernel: ap = its first row at the
// step's first k, n = valid k in the step, nrow = valid rows.  FULL: n and
// nrow are whole, no test inside.  Both forms add in the same order.
template <typename T, int VEC, bool FULL>
__device__ __forceinline__ void gemv_row_step(
    const T *__restrict__ ap, int64_t a_rs, const T *xs, int lane, int n,
    int nrow, T (&acc)[GEMV_ROW_R / 4]) {
    constexpr int RW = GEMV_ROW_R / 4;
#pragma unroll 4
    for (int j = 0; j < GEMV_ROW_S / (64 * VEC); ++j) {
        const int kk = (j * 64 + lane) * VEC;
        const int valid = FULL ? VEC : n - kk;
        if (valid >= VEC) {
            T xv[VEC], av[RW][VEC];
            gemv_ld<T, VEC>(xs + kk, xv);
#pragma unroll
            for (int r = 0; r < RW; ++r)
                if (FULL || r < nrow)
                    gemv_ld<T, VEC>(ap + r * a_rs + kk, av[r]);
#pragma unroll
            for (int r = 0; r < RW; ++r)
                if (FULL || r < nrow)
#pragma unroll
                    for (int i = 0; i < VEC; ++i) acc[r] += av[r][i] * xv[i];
        } else {
#pragma unroll
            for (int r = 0; r < RW; ++r)
                if (r < nrow)
#pragma unroll
                    for (int i = 0; i < VEC; ++i)
                        if (i < valid)
                            acc[r] += ap[r * a_rs + kk + i] * xs[kk + i];
        }
    }
}

template <typename T, bool VECP>
__global__ __launch_bounds__(256) GEMM_NO_PK_F32 void gemv_row_kernel(
    T *__restrict__ y, const T *__restrict__ a, const T *__restrict__ x,
    T *__restrict__ part, GemvArgs g) {
    constexpr int VEC = VECP ? 16 / (int)sizeof(T) : 1;
    constexpr int RW = GEMV_ROW_R / 4, S = GEMV_ROW_S;
    __shared__ __attribute__((aligned(16))) T xs[S];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t kb = (int64_t)blockIdx.y * g.klen;
    const int64_t ke = kb + g.klen < g.K ? kb + g.klen : g.K;
    const int64_t nrb = (g.M + GEMV_ROW_R - 1) / GEMV_ROW_R;
    for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
        const int64_t r0 = rb * GEMV_ROW_R + wave * RW;
        const int nrow = r0 >= g.M ? 0 : g.M - r0 < RW ? (int)(g.M - r0) : RW;
        T acc[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) acc[r] = T(0);
        for (int64_t k0 = kb; k0 < ke; k0 += S) {
            const int n = ke - k0 < S ? (int)(ke - k0) : S;
            for (int i = t; i < n; i += 256) xs[i] = x[(k0 + i) * g.x_s];
            __syncthreads();
            if (nrow > 0) {
                const T *ap = a + r0 * g.a_rs + k0;
                if (n == S && nrow == RW)
                    gemv_row_step<T, VEC, true>(ap, g.a_rs, xs, lane, n, nrow,
                                                acc);
                else
                    gemv_row_step<T, VEC, false>(ap, g.a_rs, xs, lane, n,
                                                 nrow, acc);
            }
            __syncthreads();        // the next step overwrites xs
        }
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            T v = acc[r];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0 && r < nrow) gemv_store<T>(y, part, g, r0 + r, v);
        }
    }
}

template <typename T, bool VECP>
__global__ __launch_bounds__(256) GEMM_NO_PK_F32 void gemv_col_kernel(
    T *__restrict__ y, const T *__restrict__ a, const T *__restrict__ x,
    T *__restrict__ part, GemvArgs g) {
    constexpr int VEC = VECP ? 16 / (int)sizeof(T) : 1;
    constexpr int TM = 256 / VEC, KG = VEC, R = GEMV_COL_R, S = GEMV_COL_S;
    __shared__ T xs[S];
    __shared__ T red[KG > 1 ? (KG - 1) * R : 1];
    const int t = threadIdx.x, tm = t % TM, kg = t / TM;
    const int64_t kb = (int64_t)blockIdx.y * g.klen;
    const int64_t ke = kb + g.klen < g.K ? kb + g.klen : g.K;
    const int64_t nrb = (g.M + R - 1) / R;
    for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
        const int64_t m0 = rb * R + tm * VEC, left = g.M - m0;
        const int mv = left >= VEC ? VEC : left > 0 ? (int)left : 0;
        T acc[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = T(0);
        for (int64_t k0 = kb; k0 < ke; k0 += S) {
            const int n = ke - k0 < S ? (int)(ke - k0) : S;
            for (int i = t; i < n; i += 256) xs[i] = x[(k0 + i) * g.x_s];
            __syncthreads();
            if (mv == VEC) {
                const T *ak = a + m0 * g.a_rs + k0 * g.a_cs;
#pragma unroll 8
                for (int kk = kg; kk < n; kk += KG) {
                    T av[VEC];
                    gemv_ld<T, VEC>(ak + kk * g.a_cs, av);
                    const T xv = xs[kk];
#pragma unroll
                    for (int i = 0; i < VEC; ++i) acc[i] += av[i] * xv;
                }
            } else if (mv > 0) {    // the last outputs of M, element-wise
                const T *ak = a + m0 * g.a_rs + k0 * g.a_cs;
                for (int kk = kg; kk < n; kk += KG)
#pragma unroll
                    for (int i = 0; i < VEC; ++i)
                        if (i < mv)
                            acc[i] += ak[kk * g.a_cs + i * g.a_rs] * xs[kk];
            }
            __syncthreads();        // the next step overwrites xs
        }
        if constexpr (KG > 1) {
            if (kg > 0)
#pragma unroll
                for (int i = 0; i < VEC; ++i)
                    red[(kg - 1) * R + tm * VEC + i] = acc[i];
            __syncthreads();
            if (kg == 0)
                for (int q = 1; q < KG; ++q)
#pragma unroll
                    for (int i = 0; i < VEC; ++i)
                        acc[i] += red[(q - 1) * R + tm * VEC + i];
            __syncthreads();        // the next row block overwrites red
        }
        if (kg == 0)
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                if (i < mv) gemv_store<T>(y, part, g, m0 + i, acc[i]);
    }
}

// y[m] (+)= part[0][m] + part[1][m] + ...; nparts == 0 zero-fills (K == 0).
template <typename T>
__global__ __launch_bounds__(256) GEMM_NO_PK_F32 void gemv_finish_kernel(
    T *__restrict__ y, const T *__restrict__ part, int64_t M, int64_t y_s,
    int64_t nparts, int accumulate) {
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M;
         m += (int64_t)gridDim.x * 256) {
        T v = T(0);
        for (int64_t p = 0; p < nparts; ++p) v += part[p * M + m];
        T *q = y + m * y_s;
        *q = accumulate ? *q + v : v;
    }
}

int gemv_regime(const void *a, int64_t a_rs, int64_t a_cs, int dtype) {
    const int64_t per = dtype == RT_F64 ? 2 : 4;
    const bool al = reinterpret_cast<uintptr_t>(a) % 16 == 0;
    if (a_cs == 1)
        return al && a_rs % per == 0 ? GEMV_ROW_VEC : GEMV_ROW_ELEM;
    return a_rs == 1 && al && a_cs % per == 0 ? GEMV_COL_VEC : GEMV_COL_ELEM;
}

void gemv_geometry(int regime, int64_t *rows, int64_t *step) {
    const bool row = regime == GEMV_ROW_VEC || regime == GEMV_ROW_ELEM;
    *rows = row ? (int64_t)GEMV_ROW_R : (int64_t)GEMV_COL_R;
    *step = row ? (int64_t)GEMV_ROW_S : (int64_t)GEMV_COL_S;
}

// The checks rt_gemv and rt_gemv_plan share.
int gemv_check(const char *who, int64_t M, int64_t K, int dtype) {
    if (dtype != RT_F64 && dtype != RT_F32) return fail(who, "bad dtype");
    if (M < 0 || K < 0) return fail(who, "negative extent (M/K)");
    const int64_t lim = 1LL << 40, plim = 1LL << 46;
    if (M >= lim || K >= lim) return fail(who, "extent out of range (M/K)");
    if (K && M > plim / K) return fail(who, "shape too large (M*K)");
    return 0;
}

template <typename T>
int gemv_launch(uintptr_t stream, void *y, const void *a, const void *x,
                void *scratch, const GemvArgs &g, int regime,
                int64_t nparts) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int64_t rows, step;
    gemv_geometry(regime, &rows, &step);
    const int64_t nrb = (g.M + rows - 1) / rows;
    const dim3 grid((unsigned)(nrb < GEMV_GRID_CAP ? nrb : GEMV_GRID_CAP),
                    (unsigned)nparts);
#define GEMV_GO(KERNEL)                                                    \
    hipLaunchKernelGGL((KERNEL), grid, dim3(256), 0, st,                   \
                       static_cast<T *>(y), static_cast<const T *>(a),     \
                       static_cast<const T *>(x), static_cast<T *>(scratch), g)
    if (nparts == 0) {
    } else if (regime == GEMV_ROW_VEC) {
        GEMV_GO((gemv_row_kernel<T, true>));
    } else if (regime == GEMV_ROW_ELEM) {
        GEMV_GO((gemv_row_kernel<T, false>));
    } else if (regime == GEMV_COL_VEC) {
        GEMV_GO((gemv_col_kernel<T, true>));
    } else {
        GEMV_GO((gemv_col_kernel<T, false>));
    }
#undef GEMV_GO
    if (g.split || nparts == 0) {
        const int64_t fb = (g.M + 255) / 256;
        hipLaunchKernelGGL((gemv_finish_kernel<T>),
                           dim3((unsigned)(fb < GEMV_GRID_CAP ? fb
                                                              : GEMV_GRID_CAP)),
                           dim3(256), 0, st, static_cast<T *>(y),
                           static_cast<const T *>(scratch), g.M, g.y_s,
                           nparts, g.accumulate);
    }
    return launched("gemv");
}

}  // namespace

extern "C" int rt_gemv_geometry(int dtype, int regime, int *rows_per_block,
                                int *k_step) {
    const char *who = "rt_gemv_geometry";
    if (dtype != RT_F64 && dtype != RT_F32) return fail(who, "bad dtype");
    if (regime < GEMV_ROW_VEC || regime > GEMV_COL_ELEM)
        return fail(who, "bad regime");
    if (!rows_per_block || !k_step) return fail(who, "NULL output");
    int64_t rows, step;
    gemv_geometry(regime, &rows, &step);
    *rows_per_block = (int)rows;
    *k_step = (int)step;
    return 0;
}

extern "C" int rt_gemv_plan(const void *a, int64_t M, int64_t K, int64_t a_rs,
                            int64_t a_cs, int dtype, int cus, int *regime,
                            int64_t *ksplit) {
    const char *who = "rt_gemv_plan";
    if (gemv_check(who, M, K, dtype)) return 1;
    if (cus < 1) return fail(who, "bad cus");
    if (!regime || !ksplit) return fail(who, "NULL output");
    *regime = gemv_regime(a, a_rs, a_cs, dtype);
    int64_t rows, step;
    gemv_geometry(*regime, &rows, &step);
    // Split K when the row blocks alone give the chip under 4 blocks per CU,
    // as far as every range keeps at least two k steps.
    const int64_t nrb = (M + rows - 1) / rows, steps = (K + step - 1) / step;
    const int64_t want = 4 * (int64_t)cus;
    int64_t ks = 1;
    if (nrb > 0 && nrb < want) {
        ks = (want + nrb - 1) / nrb;
        if (ks > steps / 2) ks = steps / 2;
        if (ks > GEMV_MAX_SPLIT) ks = GEMV_MAX_SPLIT;
        if (ks < 1) ks = 1;
    }
    *ksplit = ks;
    return 0;
}

extern "C" int rt_gemv(uintptr_t stream, void *y, const void *a,
                       const void *x, int64_t M, int64_t K, int64_t a_rs,
                       int64_t a_cs, int64_t x_s, int64_t y_s, int dtype,
                       int accumulate, int64_t ksplit, void *scratch) {
    const char *who = "rt_gemv";
    if (gemv_check(who, M, K, dtype)) return 1;
    if (accumulate != 0 && accumulate != 1)
        return fail(who, "bad accumulate");
    if (ksplit < 1 || ksplit > GEMV_MAX_SPLIT) return fail(who, "bad ksplit");
    if (ksplit > 1 && !scratch) return fail(who, "NULL scratch");
    if (M == 0) return 0;
    if (!y) return fail(who, "NULL y");
    if (K && (!a || !x)) return fail(who, "NULL a/x");
    if (K == 0 && accumulate) return 0;
    const int regime = gemv_regime(a, a_rs, a_cs, dtype);
    int64_t rows, step;
    gemv_geometry(regime, &rows, &step);
    GemvArgs g;
    g.M = M, g.K = K, g.a_rs = a_rs, g.a_cs = a_cs, g.x_s = x_s, g.y_s = y_s;
    g.klen = ((K + ksplit - 1) / ksplit + step - 1) / step * step;
    g.accumulate = accumulate, g.split = ksplit > 1;
    const int64_t nparts = K ? (K + g.klen - 1) / g.klen : 0;
    if (dtype == RT_F64)
        return gemv_launch<double>(stream, y, a, x, scratch, g, regime,
                                   nparts);
    return gemv_launch<float>(stream, y, a, x, scratch, g, regime, nparts);
}

// ---------------------------------------------------------------------------
// Histogram / bincount: a keyed count.  One pass over a strided box (the
// rt_arg_flat addressing and load rule), every element mapped to a bin and
// counted; `counts` (int64[nbins], zeroed by the caller) is added to.
//
// Binning modes
//   INDEX    the bin is the (integer) value; values outside [0, nbins) are
//            skipped and counted in *bad.
//   UNIFORM  numpy.lib._histograms_impl restated in the edges' dtype E: drop
//            x unless first <= x <= last (NaN fails), f = ((x - first) /
//            (last - first)) * nbins with one IEEE divide and one IEEE
//            multiply, truncate, nbins -> nbins - 1, then step down if
//            x < edges[i], else up if x >= edges[i + 1] and i is not the
//            last bin.  The correction makes the bin a function of the edges
//            alone as long as the guess is within one bin of the truth.
//   EDGES    any non-decreasing float64 edges: binary search for the number
//            of edges <= x, compared in float64; the last bin is closed;
//            NaN and values outside [first, last] are dropped.
// Edges of at most HIST_EDGES_LDS_MAX values are staged in LDS; longer lists
// are read where they are (they stay in L2).
//
// Counters, by nbins (rt_hist_regime):
//   LDS_WAVE   nbins <= HIST_WAVE_MAX_BINS: each of the block's four waves
//              adds into its own uint32 LDS copy, so a hot bin is contended
//              by 64 lanes, not 256; the copies are summed at the flush.
//              4 x 2048 x 4 B = 32 KB keeps five blocks on a CU.
//   LDS_BLOCK  nbins <= HIST_BLOCK_MAX_BINS: one uint32 LDS copy per block.
//              32768 bins are 128 KB, the largest power of two inside the
//              160 KB of a gfx950 CU and the most LDS the kernel ever asks
//              for: edges are staged only below HIST_EDGES_LDS_MAX values,
//              where the counters are small.
//   GLOBAL     64-bit atomic adds straight on counts.
// A block flushes only its nonzero LDS bins, with 64-bit global atomic adds
// (integer adds: any order gives the same counts).  The grid is capped at
// HIST_GRID_CAP blocks, so the flush is at most grid x nbins adds.  A launch
// covers at most HIST_LAUNCH_TRIPS load units per lane, i.e. at most 2^31
// elements per block, so a uint32 LDS counter cannot wrap; longer boxes take
// several launches.
//
// Wave pre-aggregation: when every active lane of a wave holds the same bin
// (sorted or constant data), one lane adds the lane count; any other mix of
// bins adds lane by lane.  The test is two readfirstlanes and a ballot per
// element.  -DHIST_PREAGG=0 builds the kernel without it, to measure it
// (tools/bench_hist.py --lib).
// ---------------------------------------------------------------------------

#ifndef HIST_PREAGG
#define HIST_PREAGG 1
#endif

namespace {

enum { HIST_INDEX = 0, HIST_UNIFORM = 1, HIST_EDGES = 2 };
enum { HIST_LDS_WAVE = 0, HIST_LDS_BLOCK = 1, HIST_GLOBAL = 2 };
enum {
    HIST_GRID_CAP = 2048,          // 256 CUs x 8 blocks, as ARG_GRID_CAP
    HIST_WAVE_MAX_BINS = 2048,
    HIST_BLOCK_MAX_BINS = 32768,
    HIST_EDGES_LDS_MAX = 4096,     // edge values (32 KB of float64)
    HIST_LAUNCH_TRIPS = 1 << 19    // x 256 lanes x 16 elements = 2^31
};

struct HistArgs {
    int64_t u0, u1;          // this launch's load units [u0, u1)
    int64_t shp[4];          // extents, right-aligned; innermost in units
    int64_t str[4];          // strides in load units
    int64_t tail0, tailn;    // 1-D 16-byte path: elements past the last unit
    int64_t nbins;
    int nd, regime, stage_edges;
};

int hist_regime(int64_t nbins) {
    return nbins <= HIST_WAVE_MAX_BINS    ? HIST_LDS_WAVE
           : nbins <= HIST_BLOCK_MAX_BINS ? HIST_LDS_BLOCK
                                          : HIST_GLOBAL;
}

__device__ __forceinline__ int64_t hist_unit_off(const HistArgs &a,
                                                 int64_t u) {
    if (a.nd == 1) return u * a.str[3];
    uint64_t rem = (uint64_t)u;
    int64_t off = 0;
#pragma unroll
    for (int d = 3; d >= 0; --d) {
        if (d < 4 - a.nd) break;      // the axes the host left after merging
        const uint64_t q = rem / (uint64_t)a.shp[d];
        off += (int64_t)(rem - q * (uint64_t)a.shp[d]) * a.str[d];
        rem = q;
    }
    return off;
}

// Where a lane's counts go: its wave's (or block's) LDS copy, or counts.
struct HistSink {
    uint32_t *lds;                 // nullptr in the GLOBAL regime
    unsigned long long *counts;
    int64_t nbins;

    __device__ __forceinline__ void add(int64_t b, uint32_t k) const {
        if (lds)
            atomicAdd(&lds[b], k);
        else
            atomicAdd(&counts[b], (unsigned long long)k);
    }

    // b < 0: nothing to count.  Anything else is inside [0, nbins).  When
    // every active lane holds the same bin, the first one adds them all.
    __device__ __forceinline__ void count(int64_t b) const {
        if (HIST_PREAGG) {
            const uint64_t act = __ballot(1);
            const int64_t b0 = gemm_uniform(b);
            if (__ballot(b == b0) == act) {
                if (b0 >= 0
                    && (int)__lane_id() == __ffsll((long long)act) - 1)
                    add(b0, (uint32_t)__popcll(act));
                return;
            }
        }
        if (b >= 0) add(b, 1u);
    }
};

template <typename T>
__device__ __forceinline__ int64_t hist_bin_index(T x, int64_t nbins) {
    const int64_t v = (int64_t)x;
    return (uint64_t)v < (uint64_t)nbins ? v : -1;
}

template <typename T, typename E>
__device__ __forceinline__ int64_t hist_bin_uniform(T x, const E *edges,
                                                    int64_t nbins, E first,
                                                    E last) {
#pragma clang fp contract(off)
    const double xd = (double)x;
    if (!(xd >= (double)first && xd <= (double)last)) return -1;
    const E xe = (E)x;
    E f;
    if constexpr (sizeof(E) == 4)
        f = __fmul_rn(__fdiv_rn(xe - first, last - first), (E)nbins);
    else
        f = __dmul_rn(__ddiv_rn(xe - first, last - first), (E)nbins);
    int64_t i = (int64_t)f;
    if (i == nbins) i = nbins - 1;
    if ((uint64_t)i >= (uint64_t)nbins) return -1;   // keeps the reads inside
    if (xe < edges[i])
        --i;
    else if (xe >= edges[i + 1] && i != nbins - 1)
        ++i;
    return (uint64_t)i < (uint64_t)nbins ? i : -1;
}

template <typename T>
__device__ __forceinline__ int64_t hist_bin_edges(T x, const double *edges,
                                                  int64_t nbins, double first,
                                                  double last) {
    const double xd = (double)x;
    if (!(xd >= first && xd <= last)) return -1;
    // lo = number of edges <= x (>= 1 here); edges[nbins] == x gives
    // nbins + 1, the closed last bin
    int64_t lo = 1, hi = nbins + 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (edges[mid] <= xd)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo > nbins ? nbins - 1 : lo - 1;
}

template <typename T, typename L, typename E, int MODE>
__device__ __forceinline__ void hist_unit(const L &unit, const HistSink &sink,
                                          const E *edges, E first, E last,
                                          uint32_t &nbad) {
    constexpr int PER = sizeof(L) / sizeof(T);
    T e[PER];
    __builtin_memcpy(e, &unit, sizeof(L));
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        int64_t b;
        if constexpr (MODE == HIST_INDEX) {
            b = hist_bin_index<T>(e[j], sink.nbins);
            nbad += b < 0;
        } else if constexpr (MODE == HIST_UNIFORM) {
            b = hist_bin_uniform<T, E>(e[j], edges, sink.nbins, first, last);
        } else {
            b = hist_bin_edges<T>(e[j], edges, sink.nbins, first, last);
        }
        sink.count(b);
    }
}

// LDS layout: [staged edges, E x (nbins + 1)] [counters, uint32 x copies x
// nbins]; either part may be absent.  L = uint4 when the box takes 16-byte
// loads, else one element; two loads in flight per lane.
template <typename T, typename L, typename E, int MODE>
__global__ __launch_bounds__(256) GEMM_NO_PK_F32 void hist_kernel(
    const T *__restrict__ in, HistArgs a, const E *__restrict__ edges,
    unsigned long long *__restrict__ counts, unsigned int *__restrict__ bad) {
    extern __shared__ __align__(16) unsigned char hist_lds[];
    const int tid = threadIdx.x;
    const int64_t nbins = a.nbins;
    E first = E(0), last = E(0);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(hist_lds);
    if constexpr (MODE != HIST_INDEX) {
        first = edges[0];
        last = edges[nbins];
        if (a.stage_edges) {
            E *se = reinterpret_cast<E *>(hist_lds);
            for (int64_t k = tid; k <= nbins; k += 256) se[k] = edges[k];
            // counters start on the next 8-byte boundary
            cnt = reinterpret_cast<uint32_t *>(
                hist_lds + (((nbins + 1) * sizeof(E) + 7) & ~(size_t)7));
            edges = se;
        }
    }
    const int copies = a.regime == HIST_LDS_WAVE    ? 4
                       : a.regime == HIST_LDS_BLOCK ? 1
                                                    : 0;
    for (int64_t k = tid; k < copies * nbins; k += 256) cnt[k] = 0u;
    __syncthreads();

    HistSink sink;
    sink.lds = copies == 0   ? nullptr
               : copies == 4 ? cnt + (tid >> 6) * nbins
                             : cnt;
    sink.counts = counts;
    sink.nbins = nbins;
    uint32_t nbad = 0;

    const L *src = reinterpret_cast<const L *>(in);
    const int64_t S = (int64_t)gridDim.x * 256;
    int64_t u = a.u0 + (int64_t)blockIdx.x * 256 + tid;
    for (; u + S < a.u1; u += 2 * S) {
        const L x0 = src[hist_unit_off(a, u)];
        const L x1 = src[hist_unit_off(a, u + S)];
        hist_unit<T, L, E, MODE>(x0, sink, edges, first, last, nbad);
        hist_unit<T, L, E, MODE>(x1, sink, edges, first, last, nbad);
    }
    if (u < a.u1) {
        const L x0 = src[hist_unit_off(a, u)];
        hist_unit<T, L, E, MODE>(x0, sink, edges, first, last, nbad);
    }
    const int64_t t = (int64_t)blockIdx.x * 256 + tid;
    if (a.u0 == 0 && t < a.tailn)
        hist_unit<T, T, E, MODE>(in[a.tail0 + t], sink, edges, first, last,
                                 nbad);
    if (MODE == HIST_INDEX && nbad && bad) atomicAdd(bad, nbad);

    if (copies) {
        __syncthreads();
        for (int64_t b = tid; b < nbins; b += 256) {
            uint32_t v = 0;
            for (int c = 0; c < copies; ++c) v += cnt[c * nbins + b];
            if (v) atomicAdd(&counts[b], (unsigned long long)v);
        }
    }
}

size_t hist_lds_bytes(int64_t nbins, int regime, bool stage, int edge_size) {
    const size_t e = stage ? ((size_t)(nbins + 1) * edge_size + 7) & ~(size_t)7
                           : 0;
    const size_t copies = regime == HIST_LDS_WAVE    ? 4
                          : regime == HIST_LDS_BLOCK ? 1
                                                     : 0;
    return e + copies * (size_t)nbins * sizeof(uint32_t);
}

template <typename T, typename L, typename E, int MODE>
int hist_launch_k(uintptr_t stream, const T *src, HistArgs a, int64_t nunits,
                  const void *edges, void *counts, void *bad) {
    auto kern = hist_kernel<T, L, E, MODE>;
    const size_t lds = hist_lds_bytes(a.nbins, a.regime, a.stage_edges != 0,
                                      sizeof(E));
    // beyond 64 KB a kernel has to be granted its LDS: once per
    // instantiation, for the most it can ask (the top of LDS_BLOCK)
    if (lds > 64 * 1024) {
        static const hipError_t granted = hipFuncSetAttribute(
            reinterpret_cast<const void *>(kern),
            hipFuncAttributeMaxDynamicSharedMemorySize,
            HIST_BLOCK_MAX_BINS * (int)sizeof(uint32_t));
        HIP_CHECK(granted);
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // a launch covers at most HIST_LAUNCH_TRIPS units per lane of the capped
    // grid; the 1-D scalar tail rides on the first one (also when nunits = 0)
    const int64_t span = (int64_t)HIST_GRID_CAP * 256 * HIST_LAUNCH_TRIPS;
    for (int64_t u0 = 0; u0 == 0 || u0 < nunits; u0 += span) {
        a.u0 = u0;
        a.u1 = nunits - u0 < span ? nunits : u0 + span;
        int64_t blocks = (a.u1 - a.u0 + 255) / 256;
        if (blocks > HIST_GRID_CAP) blocks = HIST_GRID_CAP;
        if (blocks < 1) blocks = 1;
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, st,
                           src, a, static_cast<const E *>(edges),
                           static_cast<unsigned long long *>(counts),
                           static_cast<unsigned int *>(bad));
        if (launched("rt_hist")) return 1;
    }
    return 0;
}

// The walk of a box in load units, shared with rt_select_pass: fills the
// geometry fields of `a` (nd, shp, str, tail0, tailn), sets *nunits and
// returns whether the box takes 16-byte loads.
bool hist_box_args(const void *in, int64_t in_off, int nd,
                   const int64_t *shape, const int64_t *strides, int es,
                   int64_t n, HistArgs *out, int64_t *nunits_out) {
    HistArgs &a = *out;
    const bool vec = arg_flat_vec(in, in_off, nd, shape, strides, es);
    const int64_t per = vec ? 16 / (int64_t)es : 1;
    a.tail0 = a.tailn = 0;
    for (int d = 0; d < 4; ++d) {
        const int s = d - (4 - nd);
        a.shp[d] = s >= 0 ? shape[s] : 1;
        a.str[d] = s >= 0 ? strides[s] : 0;
        if (vec && d < 3) a.str[d] /= per;
    }
    int64_t nunits = n;
    if (vec) {
        a.tail0 = (a.shp[3] / per) * per;
        a.tailn = a.shp[3] - a.tail0;     // nonzero only when nd == 1
        a.shp[3] /= per;
        nunits = n / shape[nd - 1] * a.shp[3];
    }
    // merge every axis that is dense over its inner neighbour, so a
    // contiguous N-D box walks as one axis, with no division per unit
    int k = 3;
    for (int d = 2; d >= 4 - nd; --d) {
        if (a.str[d] == a.shp[k] * a.str[k]) {
            a.shp[k] *= a.shp[d];
        } else {
            --k;
            a.shp[k] = a.shp[d];
            a.str[k] = a.str[d];
        }
    }
    a.nd = 4 - k;
    *nunits_out = nunits;
    return vec;
}

template <typename T, typename L>
int hist_launch_l(uintptr_t stream, const T *src, const HistArgs &a,
                  int64_t nunits, int mode, const void *edges,
                  int edges_dtype, void *counts, void *bad) {
    if (mode == HIST_INDEX) {
        if constexpr (std::is_integral<T>::value)
            return hist_launch_k<T, L, double, HIST_INDEX>(
                stream, src, a, nunits, nullptr, counts, bad);
        return fail("rt_hist", "INDEX mode needs an integer dtype");
    }
    if (mode == HIST_EDGES)
        return hist_launch_k<T, L, double, HIST_EDGES>(stream, src, a, nunits,
                                                       edges, counts, bad);
    if (edges_dtype == RT_F32)
        return hist_launch_k<T, L, float, HIST_UNIFORM>(stream, src, a, nunits,
                                                        edges, counts, bad);
    return hist_launch_k<T, L, double, HIST_UNIFORM>(stream, src, a, nunits,
                                                     edges, counts, bad);
}

}  // namespace

extern "C" int rt_hist_regime(int64_t nbins) {
    if (nbins < 1 || nbins >= (1LL << 40)) return -1;
    return hist_regime(nbins);
}

extern "C" int rt_hist_geometry(int *grid_cap, int *block,
                                int64_t *wave_max_bins,
                                int64_t *block_max_bins,
                                int64_t *edges_lds_max) {
    if (grid_cap) *grid_cap = HIST_GRID_CAP;
    if (block) *block = 256;
    if (wave_max_bins) *wave_max_bins = HIST_WAVE_MAX_BINS;
    if (block_max_bins) *block_max_bins = HIST_BLOCK_MAX_BINS;
    if (edges_lds_max) *edges_lds_max = HIST_EDGES_LDS_MAX;
    return 0;
}

extern "C" int rt_hist(uintptr_t stream, const void *in, int64_t in_off,
                       int nd, const int64_t *shape, const int64_t *strides,
                       int dtype, int mode, const void *edges,
                       int edges_dtype, int64_t nbins, void *counts,
                       void *bad) {
    const char *who = "rt_hist";
    int64_t n;
    if (box_extents(who, nd, 1, shape, strides, strides, &n)) return 1;
    if (dtype < RT_F64 || dtype > RT_U8) return fail(who, "bad dtype");
    if (mode < HIST_INDEX || mode > HIST_EDGES) return fail(who, "bad mode");
    if (mode == HIST_INDEX && (dtype == RT_F64 || dtype == RT_F32))
        return fail(who, "INDEX mode needs an integer dtype");
    if (nbins < 1) return fail(who, "nbins < 1");
    if (nbins >= (1LL << 40)) return fail(who, "nbins out of range");
    if (mode != HIST_INDEX) {
        if (!edges) return fail(who, "NULL edges");
        if (edges_dtype != RT_F64 && !(mode == HIST_UNIFORM
                                       && edges_dtype == RT_F32))
            return fail(who, "bad edges dtype");
    }
    if (n == 0) return 0;
    if (!in) return fail(who, "NULL in");
    if (!counts) return fail(who, "NULL counts");

    return dtype_dispatch<7>(who, dtype, [&](auto t) {
        using T = decltype(t);
        HistArgs a;
        int64_t nunits;
        const bool vec = hist_box_args(in, in_off, nd, shape, strides,
                                       sizeof(T), n, &a, &nunits);
        a.nbins = nbins;
        a.regime = hist_regime(nbins);
        a.stage_edges = mode != HIST_INDEX && nbins + 1 <= HIST_EDGES_LDS_MAX;
        const T *src = static_cast<const T *>(in) + in_off;
        if (vec)
            return hist_launch_l<T, uint4>(stream, src, a, nunits, mode, edges,
                                           edges_dtype, counts, bad);
        return hist_launch_l<T, T>(stream, src, a, nunits, mode, edges,
                                   edges_dtype, counts, bad);
    });
}

// ---------------------------------------------------------------------------
// sort / argsort (numpy.sort, numpy.argsort; the reference has neither).
//
// The order is that of include/ramba_sortkey.h: every digit and comparison
// reads rt_sort_canon(raw bits), ties go to the lower position, and the
// kernels move the raw bits, so the result is NumPy's stable sort bit for bit.
//
// rt_sort, the LONG regime: a stable LSD radix sort of a dense run, 8-bit
// digits, one pass per key byte, optionally carrying an int64 payload.
//   sort_hist_k    one read of the keys builds the 256-bin histogram of every
//                  digit position, in LDS per block, flushed with 64-bit
//                  integer atomics.  The host reads the histograms back (the
//                  call's one sync) and SKIPS every pass whose digit is the
//                  same in all n keys.
//   per live pass, three launches:
//   sort_count_k   per-block digit counts, uint32, digit-major block-minor;
//   sort_scan_k    one block per digit: the digit's base is the prefix of the
//                  up-front histogram, the block scans its row of per-block
//                  counts into 64-bit offsets.  No block waits for another;
//   sort_scatter_k a block walks its contiguous range of SORT_TILE-key tiles.
//                  A wave owns 64 x SORT_KPL consecutive keys of the tile and
//                  takes them 64 at a time: the lanes holding a key's digit
//                  are found with one 64-bit ballot per digit bit, the
//                  popcount of that mask below the lane is the key's rank
//                  among them, and a per-wave LDS counter carries the digit's
//                  count from one 64-key step to the next.  The wave counters
//                  are then scanned over digits and waves (tile order), keys
//                  and payloads are reordered through LDS, and each digit's
//                  run leaves as one contiguous global write.  Lanes past n
//                  take part in every ballot and are masked out of every
//                  count and store.
// The count is NOT fused into the previous pass's scatter.  Passes ping-pong
// between the output buffer and the scratch so that the last live pass
// writes the output buffer whatever their number; with none live the run is
// copied.  The grid is capped at SORT_GRID_CAP blocks, so the counter scratch
// is at most 256 x SORT_GRID_CAP x 12 bytes.
//
// rt_sort_lines, short lines: the composite (canonical key, position) is a
// total order, so a bitonic network on it is a stable sort.
//   WAVE   len <= 64: one line per wave, four per block, one element per
//          lane, compare-exchange by __shfl_xor over the line's power of two;
//   BLOCK  len <= SORT_LINE_MAX: one line per block, keys and uint16
//          positions staged once in LDS (at most 4096 x 10 B = 40 KB).
// Padding is (all ones, position >= len): after every real element, NaN
// included, and never written.  The raw bits are re-read at the sorted
// positions when keys are asked for.
// ---------------------------------------------------------------------------

#include "../../include/ramba_sortkey.h"

namespace {

enum {
    SORT_BLOCK = 256,
    SORT_KPL = 8,                           // keys per lane
    SORT_TILE = SORT_BLOCK * SORT_KPL,
    SORT_GRID_CAP = 2048,                   // 256 CUs x 8 blocks
    SORT_WAVE_MAX = 64,
    SORT_LINE_MAX = 4096,                   // every key width
    SORT_LINES_PER_LAUNCH = 1 << 22
};

template <typename T>
using SortU = typename rt_sort_key<T>::U;

struct SortPlan {
    int64_t ntiles, tpb;    // tiles, tiles per block
    int nblocks;
};

SortPlan sort_plan(int64_t n) {
    SortPlan p;
    p.ntiles = (n + SORT_TILE - 1) / SORT_TILE;
    p.tpb = (p.ntiles + SORT_GRID_CAP - 1) / SORT_GRID_CAP;
    if (p.tpb < 1) p.tpb = 1;
    p.nblocks = (int)((p.ntiles + p.tpb - 1) / p.tpb);
    return p;
}

// byte offsets of the parts of rt_sort's scratch
struct SortScratch {
    size_t hist, offs, counts, vals, keys, total;
};

SortScratch sort_scratch(int64_t n, int ksize, bool pay) {
    const SortPlan p = sort_plan(n);
    SortScratch s;
    s.hist = 0;
    s.offs = 8 * 256 * sizeof(uint64_t);
    s.counts = s.offs + (size_t)256 * p.nblocks * sizeof(uint64_t);
    s.vals = s.counts + (size_t)256 * p.nblocks * sizeof(uint32_t);
    s.keys = s.vals + (pay ? (size_t)n * sizeof(int64_t) : 0);
    s.total = s.keys + (((size_t)n * ksize + 15) & ~(size_t)15);
    return s;
}

template <typename T>
__device__ __forceinline__ unsigned sort_digit(SortU<T> raw, int shift) {
    return (unsigned)(rt_sort_canon<T>(raw) >> shift) & 255u;
}

// One count per valid lane into cnt[d] (LDS).  When every valid lane of the
// wave holds the same digit one lane adds the lane count (constant bytes of
// small-range data).  Call from wave-uniform control flow.
__device__ __forceinline__ void sort_count_add(uint32_t *cnt, unsigned d,
                                               bool valid) {
    const unsigned long long act = __ballot(valid);
    if (act == 0) return;
    const int lead = __ffsll((long long)act) - 1;
    const unsigned d0 = (unsigned)__shfl((int)d, lead);
    if (__ballot(valid && d != d0) == 0) {
        if ((int)(threadIdx.x & 63) == lead)
            atomicAdd(&cnt[d0], (uint32_t)__popcll(act));
    } else if (valid) {
        atomicAdd(&cnt[d], 1u);
    }
}

__global__ __launch_bounds__(256) void sort_zero_k(unsigned long long *p,
                                                   int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}

// histograms of every digit position; block b reads keys [b, b+1) x per_block
template <typename T>
__global__ __launch_bounds__(256) void sort_hist_k(
    const SortU<T> *__restrict__ keys, int64_t n, int64_t per_block,
    unsigned long long *__restrict__ hist) {
    constexpr int NB = (int)sizeof(T);
    __shared__ uint32_t cnt[NB][256];
    const int t = threadIdx.x;
#pragma unroll
    for (int b = 0; b < NB; ++b) cnt[b][t] = 0;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * per_block;
    const int64_t hi = lo + per_block < n ? lo + per_block : n;
    for (int64_t i0 = lo; i0 < hi; i0 += 256) {
        const int64_t i = i0 + t;
        const bool valid = i < hi;
        const SortU<T> c = valid ? rt_sort_canon<T>(keys[i]) : (SortU<T>)0;
#pragma unroll
        for (int b = 0; b < NB; ++b)
            sort_count_add(cnt[b], (unsigned)(c >> (8 * b)) & 255u, valid);
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const uint32_t v = cnt[b][t];
        if (v) atomicAdd(&hist[b * 256 + t], (unsigned long long)v);
    }
}

// counts[d * nblocks + b]: keys of block b's tile range with digit d
template <typename T>
__global__ __launch_bounds__(256) void sort_count_k(
    const SortU<T> *__restrict__ keys, int64_t n, int64_t per_block,
    int shift, uint32_t *__restrict__ counts) {
    __shared__ uint32_t cnt[256];
    const int t = threadIdx.x;
    cnt[t] = 0;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * per_block;
    const int64_t hi = lo + per_block < n ? lo + per_block : n;
    for (int64_t i0 = lo; i0 < hi; i0 += 256) {
        const int64_t i = i0 + t;
        const bool valid = i < hi;
        const unsigned d = valid ? sort_digit<T>(keys[i], shift) : 0u;
        sort_count_add(cnt, d, valid);
    }
    __syncthreads();
    counts[(int64_t)t * gridDim.x + blockIdx.x] = cnt[t];
}

__device__ __forceinline__ unsigned long long sort_wave_incl(
    unsigned long long x, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    return x;
}

// block d: offs[d][b] = (keys with a lower digit) + (keys of digit d in the
// blocks before b).  totals: the 256 bins of this digit position.
__global__ __launch_bounds__(256) void sort_scan_k(
    const uint32_t *__restrict__ counts,
    const unsigned long long *__restrict__ totals,
    unsigned long long *__restrict__ offs, int nblocks) {
    __shared__ unsigned long long red[4], wsum[4];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int d = blockIdx.x;
    const unsigned long long h =
        sort_wave_incl(t < d ? totals[t] : 0ull, lane);
    const int per = (nblocks + 255) / 256;
    const int lo = t * per < nblocks ? t * per : nblocks;
    const int hi = lo + per < nblocks ? lo + per : nblocks;
    const uint32_t *row = counts + (int64_t)d * nblocks;
    unsigned long long s = 0;
    for (int i = lo; i < hi; ++i) s += row[i];
    const unsigned long long x = sort_wave_incl(s, lane);
    if (lane == 63) {
        red[w] = h;
        wsum[w] = x;
    }
    __syncthreads();
    unsigned long long run = red[0] + red[1] + red[2] + red[3] + x - s;
    for (int k = 0; k < w; ++k) run += wsum[k];
    unsigned long long *orow = offs + (int64_t)d * nblocks;
    for (int i = lo; i < hi; ++i) {
        orow[i] = run;
        run += row[i];
    }
}

template <typename T, bool PAY>
__global__ __launch_bounds__(256) void sort_scatter_k(
    const SortU<T> *__restrict__ kin, SortU<T> *__restrict__ kout,
    const int64_t *__restrict__ vin, int64_t *__restrict__ vout, int64_t val0,
    const unsigned long long *__restrict__ offs, int64_t n, int shift,
    int64_t tpb, int64_t ntiles) {
    using U = SortU<T>;
    constexpr int EXB = PAY ? 8 : (int)sizeof(U);
    __shared__ __attribute__((aligned(16))) unsigned char exraw[SORT_TILE * EXB];
    __shared__ uint32_t cnt[4][256];    // per wave, per digit
    __shared__ uint32_t tstart[256];    // first slot of a digit in the tile
    __shared__ uint32_t wsum[4];
    __shared__ int64_t gbase[256];      // next global slot of a digit
    U *exk = reinterpret_cast<U *>(exraw);
    int64_t *exv = reinterpret_cast<int64_t *>(exraw);
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    volatile uint32_t *wc = cnt[w];

    gbase[t] = (int64_t)offs[(int64_t)t * gridDim.x + blockIdx.x];
    const int64_t tile0 = (int64_t)blockIdx.x * tpb;
    const int64_t tile1 = tile0 + tpb < ntiles ? tile0 + tpb : ntiles;
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t base = tile * SORT_TILE;
        const int64_t first = base + w * (64 * SORT_KPL) + lane;
        cnt[0][t] = cnt[1][t] = cnt[2][t] = cnt[3][t] = 0;
        __syncthreads();

        U key[SORT_KPL];
        int64_t pv[PAY ? SORT_KPL : 1];
        uint32_t rank[SORT_KPL];
#pragma unroll
        for (int j = 0; j < SORT_KPL; ++j) {
            const int64_t i = first + j * 64;
            const bool valid = i < n;
            key[j] = valid ? kin[i] : (U)0;
            if (PAY) pv[j] = !valid ? 0 : vin ? vin[i] : val0 + i;
        }
#pragma unroll
        for (int j = 0; j < SORT_KPL; ++j) {
            const bool valid = first + j * 64 < n;
            const unsigned d = sort_digit<T>(key[j], shift);
            // lanes of this wave that are valid and hold digit d
            unsigned long long mask = __ballot(valid);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (d >> b) & 1u;
                const unsigned long long bal = __ballot(bit);
                mask &= bit ? bal : ~bal;
            }
            const uint32_t below = (uint32_t)__popcll(mask & lt_mask);
            const uint32_t prev = wc[d];
            __builtin_amdgcn_wave_barrier();
            if (valid && below == 0) wc[d] = prev + (uint32_t)__popcll(mask);
            __builtin_amdgcn_wave_barrier();
            rank[j] = prev + below;
        }
        __syncthreads();

        // digits scanned over the tile, waves in tile order within a digit
        const uint32_t c0 = cnt[0][t], c1 = cnt[1][t], c2 = cnt[2][t],
                       c3 = cnt[3][t];
        const uint32_t tot = c0 + c1 + c2 + c3;
        uint32_t x = tot;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        uint32_t excl = x - tot;
        for (int k = 0; k < w; ++k) excl += wsum[k];
        cnt[0][t] = excl;
        cnt[1][t] = excl + c0;
        cnt[2][t] = excl + c0 + c1;
        cnt[3][t] = excl + c0 + c1 + c2;
        tstart[t] = excl;
        __syncthreads();

#pragma unroll
        for (int j = 0; j < SORT_KPL; ++j) {
            if (first + j * 64 < n) {
                rank[j] += cnt[w][sort_digit<T>(key[j], shift)];
                exk[rank[j]] = key[j];
            }
        }
        __syncthreads();
        const int64_t left = n - base;
        const int nvalid = left < SORT_TILE ? (int)left : (int)SORT_TILE;
        int64_t dst[SORT_KPL];
#pragma unroll
        for (int j = 0; j < SORT_KPL; ++j) {
            const int q = j * 256 + t;
            if (q < nvalid) {
                const U k = exk[q];
                const unsigned d = sort_digit<T>(k, shift);
                dst[j] = gbase[d] + (int64_t)(q - (int)tstart[d]);
                kout[dst[j]] = k;
            }
        }
        if (PAY) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < SORT_KPL; ++j)
                if (first + j * 64 < n) exv[rank[j]] = pv[j];
            __syncthreads();
#pragma unroll
            for (int j = 0; j < SORT_KPL; ++j)
                if (j * 256 + t < nvalid) vout[dst[j]] = exv[j * 256 + t];
        }
        __syncthreads();
        gbase[t] += tot;
    }
}

// every pass skipped: the run is already in order
template <typename U>
__global__ __launch_bounds__(256) void sort_copy_k(
    const U *__restrict__ kin, U *__restrict__ kout,
    const int64_t *__restrict__ vin, int64_t *__restrict__ vout, int64_t val0,
    int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * 256) {
        kout[i] = kin[i];
        if (vout) vout[i] = vin ? vin[i] : val0 + i;
    }
}

template <typename T>
int sort_run(uintptr_t stream, const void *in, void *out, const void *vals_in,
             int64_t val0, void *vals_out, int64_t n, void *scratch,
             int *passes_run) {
    using U = SortU<T>;
    constexpr int NB = (int)sizeof(T);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool pay = vals_out != nullptr;
    const SortPlan p = sort_plan(n);
    const SortScratch s = sort_scratch(n, NB, pay);
    char *sc = static_cast<char *>(scratch);
    auto *hist = reinterpret_cast<unsigned long long *>(sc + s.hist);
    auto *offs = reinterpret_cast<unsigned long long *>(sc + s.offs);
    auto *counts = reinterpret_cast<uint32_t *>(sc + s.counts);
    const int64_t per_block = p.tpb * SORT_TILE;

    sort_zero_k<<<NB, 256, 0, st>>>(hist, NB * 256);
    sort_hist_k<T><<<p.nblocks, 256, 0, st>>>(static_cast<const U *>(in), n,
                                              per_block, hist);
    if (launched("rt_sort histogram")) return 1;
    unsigned long long host[NB * 256];
    HIP_CHECK(hipMemcpyAsync(host, hist, sizeof(host), hipMemcpyDeviceToHost,
                             st));
    HIP_CHECK(hipStreamSynchronize(st));
    int live[NB], nlive = 0;
    for (int b = 0; b < NB; ++b) {
        bool one = false;
        for (int d = 0; d < 256; ++d)
            if (host[b * 256 + d] == (unsigned long long)n) one = true;
        if (!one) live[nlive++] = b;
    }
    if (passes_run) *passes_run = nlive;

    const U *kin = static_cast<const U *>(in);
    const int64_t *vin = static_cast<const int64_t *>(vals_in);
    if (nlive == 0) {
        const int64_t want = (n + 255) / 256;
        sort_copy_k<U><<<(unsigned)(want < 4096 ? want : 4096), 256, 0, st>>>(
            kin, static_cast<U *>(out), vin,
            static_cast<int64_t *>(vals_out), val0, n);
        return launched("rt_sort copy");
    }
    for (int k = 0; k < nlive; ++k) {
        const bool to_out = ((nlive - k) & 1) != 0;
        U *kout = to_out ? static_cast<U *>(out)
                         : reinterpret_cast<U *>(sc + s.keys);
        int64_t *vout = !pay     ? nullptr
                        : to_out ? static_cast<int64_t *>(vals_out)
                                 : reinterpret_cast<int64_t *>(sc + s.vals);
        const int shift = 8 * live[k];
        sort_count_k<T><<<p.nblocks, 256, 0, st>>>(kin, n, per_block, shift,
                                                   counts);
        sort_scan_k<<<256, 256, 0, st>>>(counts, hist + live[k] * 256, offs,
                                         p.nblocks);
        if (pay)
            sort_scatter_k<T, true><<<p.nblocks, 256, 0, st>>>(
                kin, kout, vin, vout, val0, offs, n, shift, p.tpb, p.ntiles);
        else
            sort_scatter_k<T, false><<<p.nblocks, 256, 0, st>>>(
                kin, kout, nullptr, nullptr, 0, offs, n, shift, p.tpb,
                p.ntiles);
        if (launched("rt_sort pass")) return 1;
        kin = kout;
        vin = vout;
    }
    return 0;
}

template <typename U>
__device__ __forceinline__ U sort_shfl_xor(U v, int j) {
    if constexpr (sizeof(U) == 8)
        return (U)__shfl_xor((unsigned long long)v, j);
    else
        return (U)__shfl_xor((unsigned)v, j);
}

// WAVE: one line per wave.  S: the power of two >= len.
template <typename T>
__global__ __launch_bounds__(256) void sort_lines_wave_k(
    const SortU<T> *__restrict__ in, int64_t nlines, int len, int S,
    int64_t ls, int64_t es, SortU<T> *__restrict__ out_keys,
    int64_t *__restrict__ out_pos) {
    using U = SortU<T>;
    const int lane = threadIdx.x & 63;
    const int64_t line = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (line >= nlines) return;             // a whole wave leaves together
    const U *src = in + line * ls;
    U ck = lane < len ? rt_sort_canon<T>(src[lane * es]) : (U) ~(U)0;
    int pos = lane;
    for (int k = 2; k <= S; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const U ok = sort_shfl_xor<U>(ck, j);
            const int op = __shfl_xor(pos, j);
            const bool want_min = ((lane & k) == 0) == ((lane & j) == 0);
            const bool other_less = ok < ck || (ok == ck && op < pos);
            if (other_less == want_min) {
                ck = ok;
                pos = op;
            }
        }
    }
    if (lane < len) {
        if (out_keys) out_keys[line * len + lane] = src[pos * es];
        if (out_pos) out_pos[line * len + lane] = pos;
    }
}

// BLOCK: one line per block, P = the power of two >= len slots in LDS.
template <typename T>
__global__ __launch_bounds__(256) void sort_lines_block_k(
    const SortU<T> *__restrict__ in, int len, int P, int64_t ls, int64_t es,
    SortU<T> *__restrict__ out_keys, int64_t *__restrict__ out_pos) {
    using U = SortU<T>;
    extern __shared__ __attribute__((aligned(16))) unsigned char sort_lds[];
    U *ck = reinterpret_cast<U *>(sort_lds);
    uint16_t *ps = reinterpret_cast<uint16_t *>(sort_lds + (size_t)P * sizeof(U));
    const int t = threadIdx.x;
    const int64_t line = blockIdx.x;
    const U *src = in + line * ls;
    for (int q = t; q < P; q += 256) {
        ck[q] = q < len ? rt_sort_canon<T>(src[q * es]) : (U) ~(U)0;
        ps[q] = (uint16_t)q;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int idx = t; idx < (P >> 1); idx += 256) {
                const int lo = ((idx & ~(j - 1)) << 1) | (idx & (j - 1));
                const int hi = lo | j;
                const U a = ck[lo], b = ck[hi];
                const uint16_t pa = ps[lo], pb = ps[hi];
                const bool b_less = b < a || (b == a && pb < pa);
                if (b_less == ((lo & k) == 0)) {
                    ck[lo] = b;
                    ck[hi] = a;
                    ps[lo] = pb;
                    ps[hi] = pa;
                }
            }
            __syncthreads();
        }
    }
    for (int q = t; q < len; q += 256) {
        const int pos = ps[q];
        if (out_keys) out_keys[line * len + q] = src[pos * es];
        if (out_pos) out_pos[line * len + q] = pos;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void sort_bounds_k(
    const SortU<T> *__restrict__ run, int64_t n,
    const SortU<T> *__restrict__ spl, int64_t m, int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const SortU<T> s = rt_sort_canon<T>(spl[i]);
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (rt_sort_canon<T>(run[mid]) < s)
            lo = mid + 1;
        else
            hi = mid;
    }
    out[i] = lo;
}

int sort_pow2(int64_t len) {
    int p = 1;
    while (p < len) p <<= 1;
    return p;
}

}  // namespace

extern "C" int rt_sort_geometry(int *block, int *keys_per_lane, int *grid_cap,
                                int *wave_max, int64_t *lines_per_launch,
                                int64_t *line_max) {
    if (block) *block = SORT_BLOCK;
    if (keys_per_lane) *keys_per_lane = SORT_KPL;
    if (grid_cap) *grid_cap = SORT_GRID_CAP;
    if (wave_max) *wave_max = SORT_WAVE_MAX;
    if (lines_per_launch) *lines_per_launch = SORT_LINES_PER_LAUNCH;
    if (line_max)
        for (int k = 0; k < 4; ++k) line_max[k] = SORT_LINE_MAX;
    return 0;
}

extern "C" int64_t rt_sort_scratch(int64_t n, int dtype, int with_payload) {
    if (n < 0 || n >= (1LL << 40) || dtype < RT_F64 || dtype > RT_U8)
        return -1;
    return (int64_t)sort_scratch(n, dtype_size(dtype), with_payload != 0)
        .total;
}

extern "C" int rt_sort(uintptr_t stream, const void *in, void *out,
                       const void *vals_in, int64_t val0, void *vals_out,
                       int64_t n, int dtype, void *scratch,
                       int64_t scratch_bytes, int *passes_run) {
    const char *who = "rt_sort";
    if (dtype < RT_F64 || dtype > RT_U8) return fail(who, "bad dtype");
    if (n < 0) return fail(who, "negative n");
    if (n >= (1LL << 40)) return fail(who, "n out of range");
    if (passes_run) *passes_run = 0;
    if (n == 0) return 0;
    if (!in) return fail(who, "NULL in");
    if (!out) return fail(who, "NULL out");
    if (!scratch) return fail(who, "NULL scratch");
    if (reinterpret_cast<uintptr_t>(scratch) & 15)
        return fail(who, "scratch not 16-byte aligned");
    if (scratch_bytes < rt_sort_scratch(n, dtype, vals_out != nullptr))
        return fail(who, "scratch_bytes too small (rt_sort_scratch)");
    return dtype_dispatch<7>(who, dtype, [&](auto t) {
        return sort_run<decltype(t)>(stream, in, out, vals_in, val0, vals_out,
                                     n, scratch, passes_run);
    });
}

extern "C" int rt_sort_lines(uintptr_t stream, const void *in, int64_t in_off,
                             int64_t nlines, int64_t len, int64_t line_stride,
                             int64_t elem_stride, int dtype, void *out_keys,
                             void *out_pos) {
    const char *who = "rt_sort_lines";
    if (dtype < RT_F64 || dtype > RT_U8) return fail(who, "bad dtype");
    if (nlines < 0) return fail(who, "negative nlines");
    if (len < 0) return fail(who, "negative len");
    if (nlines >= (1LL << 40)) return fail(who, "nlines out of range");
    if (len > SORT_LINE_MAX) return fail(who, "len exceeds line_max");
    if (nlines == 0 || len == 0) return 0;
    if (nlines > (1LL << 46) / len)
        return fail(who, "nlines x len too large");
    if (!in) return fail(who, "NULL in");
    if (!out_keys && !out_pos) return fail(who, "NULL out_keys and out_pos");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dtype_dispatch<7>(who, dtype, [&](auto t) {
        using T = decltype(t);
        using U = SortU<T>;
        const int P = sort_pow2(len);
        for (int64_t l0 = 0; l0 < nlines; l0 += SORT_LINES_PER_LAUNCH) {
            const int64_t nl = nlines - l0 < SORT_LINES_PER_LAUNCH
                                   ? nlines - l0
                                   : (int64_t)SORT_LINES_PER_LAUNCH;
            const U *src = static_cast<const U *>(in) + in_off
                           + l0 * line_stride;
            U *ok = out_keys ? static_cast<U *>(out_keys) + l0 * len : nullptr;
            int64_t *op =
                out_pos ? static_cast<int64_t *>(out_pos) + l0 * len : nullptr;
            if (len <= SORT_WAVE_MAX)
                sort_lines_wave_k<T><<<(unsigned)((nl + 3) / 4), 256, 0, st>>>(
                    src, nl, (int)len, P, line_stride, elem_stride, ok, op);
            else
                sort_lines_block_k<T>
                    <<<(unsigned)nl, 256, (size_t)P * (sizeof(U) + 2), st>>>(
                        src, (int)len, P, line_stride, elem_stride, ok, op);
        }
        return launched(who);
    });
}

extern "C" int rt_sort_bounds(uintptr_t stream, const void *run, int64_t n,
                              int dtype, const void *splitters, int64_t m,
                              void *bounds) {
    const char *who = "rt_sort_bounds";
    if (dtype < RT_F64 || dtype > RT_U8) return fail(who, "bad dtype");
    if (n < 0 || n >= (1LL << 40)) return fail(who, "n out of range");
    if (m < 0 || m >= (1LL << 31)) return fail(who, "m out of range");
    if (m == 0) return 0;
    if (n > 0 && !run) return fail(who, "NULL run");
    if (!splitters) return fail(who, "NULL splitters");
    if (!bounds) return fail(who, "NULL bounds");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dtype_dispatch<7>(who, dtype, [&](auto t) {
        using T = decltype(t);
        sort_bounds_k<T><<<(unsigned)((m + 255) / 256), 256, 0, st>>>(
            static_cast<const SortU<T> *>(run), n,
            static_cast<const SortU<T> *>(splitters), m,
            static_cast<int64_t *>(bounds));
        return launched(who);
    });
}

// ---------------------------------------------------------------------------
// Order statistics (numpy.median / percentile / quantile; the reference has
// none): rt_select_pass, one MSD pass of a radix select over the canonical
// key of ramba_sortkey.h.
//
// A selection only has to know how many keys fall in each digit bin below
// the prefixes already decided, so a pass is a keyed count that moves no
// data: every element's key is compared with up to SELECT_NQ_MAX distinct
// prefixes (kernel arguments, copied into LDS once per block so that they
// hold no scalar registers through the loop) and the one it matches, if
// any, gets a count in that prefix's 256 bins.  The box is
// walked as rt_hist walks it (hist_box_args, hist_unit_off: 16-byte loads
// under the rt_arg_flat rule, two loads in flight per lane, the capped grid,
// at most 2^31 elements per block and launch).
//
// Counters: uint32[nq][256] in LDS per wave of the 256-lane block (32 KB at
// nq = 8), summed and flushed with 64-bit atomic adds of the nonzero bins.
// The top pass of real float data is one hot bin, so the wave rule of
// rt_hist applies: when every active lane holds the same (prefix, digit),
// or none matches, one lane adds the lane count (or nothing is added).
// After the first narrowing almost no lane matches and the pass is a
// streaming read.
//
// Collect: with a buffer, each wave stages the keys that matched in its own
// LDS (ballot, popcount, the lane's rank among the matching lanes) and
// appends SELECT_STAGE of them at a time with one atomic add on the cursor;
// scattered matches would otherwise queue on that one address.  A slot at
// or past collect_cap is not written.  Later passes read that buffer with
// CANON set, which skips the transform.
// Everything written is an integer count or a key whose position does not
// matter, so results are the same from run to run.
// ---------------------------------------------------------------------------

namespace {

enum { SELECT_NQ_MAX = 8, SELECT_DIGIT_BITS = 8, SELECT_STAGE = 256 };

struct SelectArgs {
    HistArgs box;                    // the walk; the binning fields are unused
    uint64_t pre[SELECT_NQ_MAX];     // the decided high bits, in place
    uint64_t mask;                   // the key bits above shift + 8
    int64_t cap;                     // collect capacity, in keys
    int shift, nq;
};

// the rt_hist wave rule on a wave's LDS copy; b < 0: nothing to count
__device__ __forceinline__ void select_count(uint32_t *cnt, int b) {
    const uint64_t act = __ballot(1);
    const int b0 = __builtin_amdgcn_readfirstlane(b);
    if (__ballot(b == b0) == act) {
        if (b0 >= 0 && (int)__lane_id() == __ffsll((long long)act) - 1)
            atomicAdd(&cnt[b0], (uint32_t)__popcll(act));
        return;
    }
    if (b >= 0) atomicAdd(&cnt[b], 1u);
}

// A wave's staged keys go to the collect buffer with ONE atomic add on the
// cursor; run by whichever lanes of the wave are active.  `stage` and
// `staged` are the wave's own LDS, volatile so that the accesses of one wave,
// which the hardware performs in order, also stay in program order.
template <typename U>
__device__ __forceinline__ void select_flush(
    volatile U *stage, volatile int *staged, int64_t cap,
    U *__restrict__ collect, unsigned long long *__restrict__ cursor) {
    const uint64_t act = __ballot(1);
    const int lane = (int)__lane_id();
    const int n = *staged;
    int64_t base = 0;
    if (lane == __ffsll((long long)act) - 1)
        base = (int64_t)atomicAdd(cursor, (unsigned long long)n);
    base = gemm_uniform(base);                  // the first active lane's
    for (int i = __popcll(act & (((uint64_t)1 << lane) - 1)); i < n;
         i += __popcll(act))
        if (base + i < cap) collect[base + i] = stage[i];
    if (lane == __ffsll((long long)act) - 1) *staged = 0;
}

template <typename T, typename L, bool CANON>
__device__ __forceinline__ void select_unit(
    const L &unit, const SelectArgs &s, const uint64_t *pre, uint32_t *cnt,
    uint32_t &nnan, volatile typename rt_sort_key<T>::U *stage,
    volatile int *staged, typename rt_sort_key<T>::U *__restrict__ collect,
    unsigned long long *__restrict__ cursor) {
    typedef typename rt_sort_key<T>::U U;
    constexpr int PER = sizeof(L) / sizeof(U);
    U e[PER];
    __builtin_memcpy(e, &unit, sizeof(L));
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const U key = CANON ? e[j] : rt_sort_canon<T>(e[j]);
        if (rt_sort_key<T>::FLT && !CANON) nnan += key == (U) ~(U)0;
        const uint64_t hi = (uint64_t)key & s.mask;
        int q = -1;
#pragma nounroll
        for (int k = 0; k < s.nq; ++k)
            if (hi == pre[k]) q = k;
        select_count(cnt, q < 0 ? -1
                                : q * 256 + (int)(((uint64_t)key >> s.shift)
                                                  & 255));
        if (collect) {
            const uint64_t m = __ballot(q >= 0);
            if (m) {
                const int add = __popcll(m);
                if (*staged + add > SELECT_STAGE)
                    select_flush<U>(stage, staged, s.cap, collect, cursor);
                const int at = *staged;
                if (q >= 0)
                    stage[at + __popcll(m & (((uint64_t)1 << __lane_id())
                                             - 1))] = key;
                if ((int)__lane_id() == __ffsll((long long)m) - 1)
                    *staged = at + add;
            }
        }
    }
}

// L = uint4 when the box takes 16-byte loads, else one key
template <typename T, typename L, bool CANON>
__global__ __launch_bounds__(256) void select_kernel(
    const typename rt_sort_key<T>::U *__restrict__ in, SelectArgs s,
    unsigned long long *__restrict__ counts,
    unsigned long long *__restrict__ nan_count,
    typename rt_sort_key<T>::U *__restrict__ collect,
    unsigned long long *__restrict__ cursor) {
    typedef typename rt_sort_key<T>::U U;
    extern __shared__ __align__(16) unsigned char select_lds[];
    // LDS: the prefixes (read per element, so that they hold no scalar
    // registers through the loop), then the four waves' counters
    uint64_t *pre = reinterpret_cast<uint64_t *>(select_lds);
    uint32_t *all = reinterpret_cast<uint32_t *>(pre + SELECT_NQ_MAX);
    const int tid = threadIdx.x;
    const int nb = s.nq * 256;
    // when collecting: each wave's count of staged keys, and its stage
    int *nst = reinterpret_cast<int *>(all + 4 * nb);
    volatile int *staged = nst + (tid >> 6);
    volatile U *stage = reinterpret_cast<U *>(nst + 4)
                        + (tid >> 6) * SELECT_STAGE;
    if (tid < SELECT_NQ_MAX) pre[tid] = s.pre[tid];
    if (collect && tid < 4) nst[tid] = 0;
    for (int k = tid; k < 4 * nb; k += 256) all[k] = 0u;
    __syncthreads();
    uint32_t *cnt = all + (tid >> 6) * nb;
    uint32_t nnan = 0;

    const HistArgs &a = s.box;
    const L *src = reinterpret_cast<const L *>(in);
    const int64_t S = (int64_t)gridDim.x * 256;
    int64_t u = a.u0 + (int64_t)blockIdx.x * 256 + tid;
    for (; u + S < a.u1; u += 2 * S) {
        const L x0 = src[hist_unit_off(a, u)];
        const L x1 = src[hist_unit_off(a, u + S)];
        select_unit<T, L, CANON>(x0, s, pre, cnt, nnan, stage, staged, collect,
                                 cursor);
        select_unit<T, L, CANON>(x1, s, pre, cnt, nnan, stage, staged, collect,
                                 cursor);
    }
    if (u < a.u1) {
        const L x0 = src[hist_unit_off(a, u)];
        select_unit<T, L, CANON>(x0, s, pre, cnt, nnan, stage, staged, collect,
                                 cursor);
    }
    const int64_t t = (int64_t)blockIdx.x * 256 + tid;
    if (a.u0 == 0 && t < a.tailn)
        select_unit<T, U, CANON>(in[a.tail0 + t], s, pre, cnt, nnan, stage,
                                 staged, collect, cursor);
    if (collect && *staged)         // the whole wave is here again
        select_flush<U>(stage, staged, s.cap, collect, cursor);
    if (rt_sort_key<T>::FLT && !CANON && nnan && nan_count)
        atomicAdd(nan_count, (unsigned long long)nnan);

    __syncthreads();
    for (int b = tid; b < nb; b += 256) {
        const uint32_t v = all[b] + all[nb + b] + all[2 * nb + b]
                           + all[3 * nb + b];
        if (v) atomicAdd(&counts[b], (unsigned long long)v);
    }
}

template <typename T, typename L, bool CANON>
int select_launch(uintptr_t stream, const void *src, SelectArgs s,
                  int64_t nunits, void *counts, void *nan_count,
                  void *collect, void *cursor) {
    typedef typename rt_sort_key<T>::U U;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = SELECT_NQ_MAX * sizeof(uint64_t)
                       + (size_t)4 * s.nq * 256 * sizeof(uint32_t)
                       + (collect ? 4 * sizeof(int)
                                        + 4 * SELECT_STAGE * sizeof(U)
                                  : 0);
    // as rt_hist: a launch covers at most HIST_LAUNCH_TRIPS units per lane
    // of the capped grid, and the 1-D scalar tail rides on the first one
    const int64_t span = (int64_t)HIST_GRID_CAP * 256 * HIST_LAUNCH_TRIPS;
    for (int64_t u0 = 0; u0 == 0 || u0 < nunits; u0 += span) {
        s.box.u0 = u0;
        s.box.u1 = nunits - u0 < span ? nunits : u0 + span;
        int64_t blocks = (s.box.u1 - s.box.u0 + 255) / 256;
        if (blocks > HIST_GRID_CAP) blocks = HIST_GRID_CAP;
        if (blocks < 1) blocks = 1;
        hipLaunchKernelGGL((select_kernel<T, L, CANON>),
                           dim3((unsigned)blocks), dim3(256), lds, st,
                           static_cast<const U *>(src), s,
                           static_cast<unsigned long long *>(counts),
                           static_cast<unsigned long long *>(nan_count),
                           static_cast<U *>(collect),
                           static_cast<unsigned long long *>(cursor));
        if (launched("rt_select_pass")) return 1;
    }
    return 0;
}

}  // namespace

extern "C" int rt_select_geometry(int *grid_cap, int *block, int *nq_max,
                                  int *digit_bits) {
    if (grid_cap) *grid_cap = HIST_GRID_CAP;
    if (block) *block = 256;
    if (nq_max) *nq_max = SELECT_NQ_MAX;
    if (digit_bits) *digit_bits = SELECT_DIGIT_BITS;
    return 0;
}

extern "C" int rt_select_pass(uintptr_t stream, const void *in,
                              int64_t in_off, int nd, const int64_t *shape,
                              const int64_t *strides, int dtype,
                              int canonical, int shift, int nq,
                              const uint64_t *prefixes, void *counts,
                              void *nan_count, void *collect_buf,
                              int64_t collect_cap, void *cursor) {
    const char *who = "rt_select_pass";
    int64_t n;
    if (box_extents(who, nd, 1, shape, strides, strides, &n)) return 1;
    if (dtype < RT_F64 || dtype > RT_U8) return fail(who, "bad dtype");
    const int width = 8 * dtype_size(dtype);
    if (shift < 0 || shift % SELECT_DIGIT_BITS
        || shift + SELECT_DIGIT_BITS > width)
        return fail(who, "bad shift");
    if (nq < 1 || nq > SELECT_NQ_MAX) return fail(who, "nq out of range");
    if (!prefixes) return fail(who, "NULL prefixes");
    const int top = shift + SELECT_DIGIT_BITS;      // bits below: undecided
    const uint64_t keymask = width == 64 ? ~(uint64_t)0
                                         : ((uint64_t)1 << width) - 1;
    const uint64_t mask = top >= 64 ? 0 : keymask >> top << top;
    for (int q = 0; q < nq; ++q) {
        if (prefixes[q] & ~mask)
            return fail(who, "prefix has bits outside the decided digits");
        for (int p = 0; p < q; ++p)
            if (prefixes[p] == prefixes[q])
                return fail(who, "duplicate prefix");
    }
    if (collect_cap < 0) return fail(who, "negative collect_cap");
    if (collect_buf && !cursor)
        return fail(who, "collect buffer without a cursor");
    if (canonical && (nd != 1 || strides[0] != 1))
        return fail(who, "canonical input must be a dense 1-D run");
    if (n == 0) return 0;
    if (!in) return fail(who, "NULL in");
    if (!counts) return fail(who, "NULL counts");

    return dtype_dispatch<7>(who, dtype, [&](auto t) {
        using T = decltype(t);
        SelectArgs s;
        int64_t nunits;
        const bool vec = hist_box_args(in, in_off, nd, shape, strides,
                                       sizeof(T), n, &s.box, &nunits);
        s.box.nbins = 0, s.box.regime = 0, s.box.stage_edges = 0;
        for (int q = 0; q < SELECT_NQ_MAX; ++q)
            s.pre[q] = q < nq ? prefixes[q] : 0;
        s.mask = mask, s.cap = collect_cap, s.shift = shift, s.nq = nq;
        const void *src = static_cast<const T *>(in) + in_off;
        if (canonical)
            return vec ? select_launch<T, uint4, true>(
                             stream, src, s, nunits, counts, nan_count,
                             collect_buf, cursor)
                       : select_launch<T, typename rt_sort_key<T>::U, true>(
                             stream, src, s, nunits, counts, nan_count,
                             collect_buf, cursor);
        return vec ? select_launch<T, uint4, false>(
                         stream, src, s, nunits, counts, nan_count,
                         collect_buf, cursor)
                   : select_launch<T, typename rt_sort_key<T>::U, false>(
                         stream, src, s, nunits, counts, nan_count,
                         collect_buf, cursor);
    });
}

// ---------------------------------------------------------------------------
// unique (numpy.unique of a sorted run; the reference has none): the
// rt_unique_* run compaction.  The input is what rt_sort leaves: a dense run
// of raw keys in the canonical order of ramba_sortkey.h, optionally with the
// int64 payloads that travelled with them.
//
// Head rule: key i is a run head iff i == 0 or rt_sort_canon(key[i]) !=
// rt_sort_canon(key[i-1]).  Nothing else decides equality, so -0.0 and +0.0
// are one value and all NaNs are one value; the head is the FIRST key of its
// run and its raw bits are what is written.
//
// Tiling (both passes): a tile is UNIQ_BLOCK x UNIQ_KPL consecutive keys and
// lane t of the block owns keys [t * KPL, (t + 1) * KPL) of it, a blocked
// arrangement, read as KPL * sizeof(key) / 16 loads of 16 bytes when the run
// is 16-byte aligned and the tile is whole (else key by key, guarded by n).
// A lane compares its keys in registers; the one neighbour across a lane
// boundary, the last key of the lane below, arrives by __shfl_up; lane 0 of a
// wave has no lane below and loads the key before its first from global
// memory, the one second load across a wave or tile boundary.  The heads of
// a lane are a KPL-bit mask.
//   uniq_count_k   block b walks its contiguous range of tiles; per key slot j
//                  one ballot of "slot j is a head", and the popcounts add up
//                  to the wave's heads.  One int64 per block.
//   uniq_scan_k    one block: the exclusive scan of the per-block counts and
//                  the total U, which the host reads back (the one stream
//                  synchronisation) to size the outputs.
//   uniq_write_k   the same walk re-flags the heads.  The heads held by the
//                  lanes below come from the same ballots (popcount under the
//                  lane mask), the waves below from a 4-entry LDS scan, the
//                  tiles before from a running count and the blocks before
//                  from the scan.  A head at run position i with slot u writes
//                  key[i] (raw), pos[i] as first[u] and i as start[u], each
//                  only when that output was asked for.
//   uniq_edge_k /  counts[u] = start[u+1] - start[u] IN PLACE, with n closing
//   uniq_diff_k    the last run: blocks own contiguous ranges of slots;
//                  uniq_edge_k first saves every range's successor start (or
//                  n), a launch boundary later uniq_diff_k walks each range
//                  front to back, reading a chunk and its successor before a
//                  barrier and writing after it.
// No kernel waits for another block and there is no atomic: every output is
// fixed by the input.
// ---------------------------------------------------------------------------

namespace {

enum {
    UNIQ_BLOCK = 256,
    UNIQ_KPL = 16,                          // keys per lane
    UNIQ_TILE = UNIQ_BLOCK * UNIQ_KPL,
    UNIQ_GRID_CAP = 2048                    // 256 CUs x 8 blocks
};

struct UniqPlan {
    int64_t ntiles, tpb;
    int nblocks;
};

UniqPlan uniq_plan(int64_t n) {
    UniqPlan p;
    p.ntiles = (n + UNIQ_TILE - 1) / UNIQ_TILE;
    p.tpb = (p.ntiles + UNIQ_GRID_CAP - 1) / UNIQ_GRID_CAP;
    if (p.tpb < 1) p.tpb = 1;
    p.nblocks = (int)((p.ntiles + p.tpb - 1) / p.tpb);
    return p;
}

// int64 slots of the scratch: counts[nblocks], base[nblocks + 1] (the last is
// U), edge[UNIQ_GRID_CAP]
int64_t uniq_scratch_bytes(int64_t n) {
    const UniqPlan p = uniq_plan(n);
    return (((int64_t)2 * p.nblocks + 1 + UNIQ_GRID_CAP) * 8 + 15) & ~15LL;
}

template <typename U>
__device__ __forceinline__ U uniq_shfl_up1(U v) {
    if constexpr (sizeof(U) == 8)
        return (U)__shfl_up((unsigned long long)v, 1);
    else
        return (U)__shfl_up((unsigned)v, 1);
}

// The lane's KPL raw keys of the tile at `base` (0 past n) and the mask of
// its heads.  VEC: the run is 16-byte aligned.  Every lane of the block must
// call (the shuffle), whatever it holds.
template <typename T, bool VEC>
__device__ __forceinline__ uint32_t uniq_heads(
    const SortU<T> *__restrict__ keys, int64_t n, int64_t base, int t,
    SortU<T> *raw) {
    using U = SortU<T>;
    const int64_t i0 = base + (int64_t)t * UNIQ_KPL;
    if (VEC && base + UNIQ_TILE <= n) {
        constexpr int NL = UNIQ_KPL * (int)sizeof(U) / 16;
        const uint4 *src = reinterpret_cast<const uint4 *>(keys + i0);
        uint4 q[NL];
#pragma unroll
        for (int k = 0; k < NL; ++k) q[k] = src[k];
        __builtin_memcpy(raw, q, sizeof(q));
    } else {
#pragma unroll
        for (int j = 0; j < UNIQ_KPL; ++j)
            raw[j] = i0 + j < n ? keys[i0 + j] : (U)0;
    }
    U c[UNIQ_KPL];
#pragma unroll
    for (int j = 0; j < UNIQ_KPL; ++j) c[j] = rt_sort_canon<T>(raw[j]);
    U prev = uniq_shfl_up1<U>(c[UNIQ_KPL - 1]);
    bool first = false;                 // no key before this lane's first
    if ((t & 63) == 0) {
        if (i0 > 0 && i0 < n)
            prev = rt_sort_canon<T>(keys[i0 - 1]);
        else
            first = true;
    }
    uint32_t heads = (i0 < n && (first || c[0] != prev)) ? 1u : 0u;
#pragma unroll
    for (int j = 1; j < UNIQ_KPL; ++j)
        heads |= (i0 + j < n && c[j] != c[j - 1]) ? (1u << j) : 0u;
    return heads;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void uniq_count_k(
    const SortU<T> *__restrict__ keys, int64_t n, int64_t tpb, int64_t ntiles,
    int64_t *__restrict__ counts) {
    __shared__ int64_t wsum[4];
    const int t = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * tpb;
    const int64_t tile1 = tile0 + tpb < ntiles ? tile0 + tpb : ntiles;
    int64_t mine = 0;                   // the wave's heads, the same in its lanes
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        SortU<T> raw[UNIQ_KPL];
        const uint32_t heads =
            uniq_heads<T, VEC>(keys, n, tile * UNIQ_TILE, t, raw);
#pragma unroll
        for (int j = 0; j < UNIQ_KPL; ++j)
            mine += __popcll(__ballot((heads >> j) & 1u));
    }
    if ((t & 63) == 0) wsum[t >> 6] = mine;
    __syncthreads();
    if (t == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one block: base[b] = counts[0] + .. + counts[b-1], base[nblocks] = U
__global__ __launch_bounds__(256) void uniq_scan_k(
    const int64_t *__restrict__ counts, int64_t *__restrict__ base,
    int nblocks) {
    __shared__ unsigned long long wsum[4];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int per = (nblocks + 255) / 256;
    const int lo = t * per < nblocks ? t * per : nblocks;
    const int hi = lo + per < nblocks ? lo + per : nblocks;
    unsigned long long s = 0;
    for (int i = lo; i < hi; ++i) s += (unsigned long long)counts[i];
    const unsigned long long x = sort_wave_incl(s, lane);
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    unsigned long long run = x - s;
    for (int k = 0; k < w; ++k) run += wsum[k];
    for (int i = lo; i < hi; ++i) {
        base[i] = (int64_t)run;
        run += (unsigned long long)counts[i];
    }
    if (t == 255) base[nblocks] = (int64_t)run;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void uniq_write_k(
    const SortU<T> *__restrict__ keys, const int64_t *__restrict__ pos,
    int64_t n, int64_t tpb, int64_t ntiles, const int64_t *__restrict__ base,
    SortU<T> *__restrict__ out_keys, int64_t *__restrict__ out_first,
    int64_t *__restrict__ out_start) {
    __shared__ int wsum[2][4];          // double-buffered: one barrier a tile
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const int64_t tile0 = (int64_t)blockIdx.x * tpb;
    const int64_t tile1 = tile0 + tpb < ntiles ? tile0 + tpb : ntiles;
    int64_t run = base[blockIdx.x];     // slots used before this tile
    int buf = 0;
    for (int64_t tile = tile0; tile < tile1; ++tile, buf ^= 1) {
        SortU<T> raw[UNIQ_KPL];
        const int64_t tbase = tile * UNIQ_TILE;
        const uint32_t heads = uniq_heads<T, VEC>(keys, n, tbase, t, raw);
        int below = 0, wave = 0;        // heads in the lanes below; in the wave
#pragma unroll
        for (int j = 0; j < UNIQ_KPL; ++j) {
            const unsigned long long b = __ballot((heads >> j) & 1u);
            below += __popcll(b & lt_mask);
            wave += __popcll(b);
        }
        if (lane == 0) wsum[buf][w] = wave;
        __syncthreads();
        int before = below, total = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int s = wsum[buf][k];
            before += k < w ? s : 0;
            total += s;
        }
        const int64_t i0 = tbase + (int64_t)t * UNIQ_KPL;
#pragma unroll
        for (int j = 0; j < UNIQ_KPL; ++j) {
            if ((heads >> j) & 1u) {
                const int64_t u =
                    run + before + __popc(heads & ((1u << j) - 1u));
                if (out_keys) out_keys[u] = raw[j];
                if (out_first) out_first[u] = pos ? pos[i0 + j] : i0 + j;
                if (out_start) out_start[u] = i0 + j;
            }
        }
        run += total;
    }
}

// The U starts are cut into at most UNIQ_GRID_CAP contiguous ranges of `per`
// slots, a multiple of 256; U is read where uniq_scan_k left it, so the host
// need not know it and the launch is UNIQ_GRID_CAP ranges wide, the ranges
// past U empty.
__device__ __forceinline__ int64_t uniq_range(int64_t nu) {
    const int64_t per = (nu + UNIQ_GRID_CAP - 1) / UNIQ_GRID_CAP;
    return (per + 255) / 256 * 256;
}

__global__ __launch_bounds__(256) void uniq_edge_k(
    const int64_t *__restrict__ start, const int64_t *__restrict__ nu_p,
    int64_t n, int64_t *__restrict__ edge) {
    const int64_t nu = *nu_p, per = uniq_range(nu);
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= UNIQ_GRID_CAP) return;
    const int64_t next = (b + 1) * per;
    edge[b] = next < nu ? start[next] : n;
}

__global__ __launch_bounds__(256) void uniq_diff_k(
    int64_t *__restrict__ start, const int64_t *__restrict__ nu_p,
    const int64_t *__restrict__ edge) {
    const int64_t nu = *nu_p, per = uniq_range(nu);
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < nu ? lo + per : nu;
    const int64_t last = edge[blockIdx.x];
    for (int64_t u0 = lo; u0 < hi; u0 += 256) {     // block-uniform bounds
        const int64_t u = u0 + threadIdx.x;
        int64_t a = 0, b = 0;
        if (u < hi) {
            a = start[u];
            b = u + 1 < hi ? start[u + 1] : last;
        }
        __syncthreads();                // every read of this chunk is done
        if (u < hi) start[u] = b - a;
    }
}

template <typename T>
int uniq_count_run(hipStream_t st, const void *keys, int64_t n, void *scratch,
                   int64_t *n_unique) {
    using U = SortU<T>;
    const UniqPlan p = uniq_plan(n);
    int64_t *counts = static_cast<int64_t *>(scratch);
    int64_t *base = counts + p.nblocks;
    const U *k = static_cast<const U *>(keys);
    if (reinterpret_cast<uintptr_t>(keys) % 16 == 0)
        uniq_count_k<T, true><<<p.nblocks, 256, 0, st>>>(k, n, p.tpb, p.ntiles,
                                                         counts);
    else
        uniq_count_k<T, false><<<p.nblocks, 256, 0, st>>>(k, n, p.tpb,
                                                          p.ntiles, counts);
    uniq_scan_k<<<1, 256, 0, st>>>(counts, base, p.nblocks);
    if (launched("rt_unique_count")) return 1;
    int64_t total = 0;
    HIP_CHECK(hipMemcpyAsync(&total, base + p.nblocks, sizeof(total),
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    *n_unique = total;
    return 0;
}

template <typename T>
int uniq_write_run(hipStream_t st, const void *keys, const void *pos,
                   int64_t n, void *scratch, void *out_keys, void *out_first,
                   void *out_counts) {
    using U = SortU<T>;
    const UniqPlan p = uniq_plan(n);
    int64_t *base = static_cast<int64_t *>(scratch) + p.nblocks;
    int64_t *edge = base + p.nblocks + 1;
    const U *k = static_cast<const U *>(keys);
    if (reinterpret_cast<uintptr_t>(keys) % 16 == 0)
        uniq_write_k<T, true><<<p.nblocks, 256, 0, st>>>(
            k, static_cast<const int64_t *>(pos), n, p.tpb, p.ntiles, base,
            static_cast<U *>(out_keys), static_cast<int64_t *>(out_first),
            static_cast<int64_t *>(out_counts));
    else
        uniq_write_k<T, false><<<p.nblocks, 256, 0, st>>>(
            k, static_cast<const int64_t *>(pos), n, p.tpb, p.ntiles, base,
            static_cast<U *>(out_keys), static_cast<int64_t *>(out_first),
            static_cast<int64_t *>(out_counts));
    if (launched("rt_unique_write")) return 1;
    if (!out_counts) return 0;
    uniq_edge_k<<<UNIQ_GRID_CAP / 256, 256, 0, st>>>(
        static_cast<int64_t *>(out_counts), base + p.nblocks, n, edge);
    uniq_diff_k<<<UNIQ_GRID_CAP, 256, 0, st>>>(
        static_cast<int64_t *>(out_counts), base + p.nblocks, edge);
    return launched("rt_unique_write counts");
}

}  // namespace

extern "C" int rt_unique_geometry(int *block, int *keys_per_lane,
                                  int *grid_cap) {
    if (block) *block = UNIQ_BLOCK;
    if (keys_per_lane) *keys_per_lane = UNIQ_KPL;
    if (grid_cap) *grid_cap = UNIQ_GRID_CAP;
    return 0;
}

extern "C" int64_t rt_unique_scratch(int64_t n) {
    if (n < 0 || n >= (1LL << 40)) return -1;
    return uniq_scratch_bytes(n);
}

namespace {

int uniq_validate(const char *who, const void *keys, int64_t n, int dtype,
                  const void *scratch) {
    if (dtype < RT_F64 || dtype > RT_U8) return fail(who, "bad dtype");
    if (n < 0) return fail(who, "negative n");
    if (n >= (1LL << 40)) return fail(who, "n out of range");
    if (n == 0) return 0;
    if (!keys) return fail(who, "NULL keys");
    if (!scratch) return fail(who, "NULL scratch");
    if (reinterpret_cast<uintptr_t>(scratch) & 15)
        return fail(who, "scratch not 16-byte aligned");
    return 0;
}

}  // namespace

extern "C" int rt_unique_count(uintptr_t stream, const void *keys, int64_t n,
                               int dtype, void *scratch,
                               int64_t scratch_bytes, int64_t *n_unique) {
    const char *who = "rt_unique_count";
    if (uniq_validate(who, keys, n, dtype, scratch)) return 1;
    if (!n_unique) return fail(who, "NULL n_unique");
    *n_unique = 0;
    if (n == 0) return 0;
    if (scratch_bytes < uniq_scratch_bytes(n))
        return fail(who, "scratch_bytes too small (rt_unique_scratch)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dtype_dispatch<7>(who, dtype, [&](auto t) {
        return uniq_count_run<decltype(t)>(st, keys, n, scratch, n_unique);
    });
}

extern "C" int rt_unique_write(uintptr_t stream, const void *keys,
                               const void *pos, int64_t n, int dtype,
                               void *scratch, void *out_keys, void *out_first,
                               void *out_counts) {
    const char *who = "rt_unique_write";
    if (uniq_validate(who, keys, n, dtype, scratch)) return 1;
    if (n == 0) return 0;
    if (!out_keys && !out_first && !out_counts)
        return fail(who, "NULL out_keys, out_first and out_counts");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dtype_dispatch<7>(who, dtype, [&](auto t) {
        return uniq_write_run<decltype(t)>(st, keys, pos, n, scratch, out_keys,
                                           out_first, out_counts);
    });
}

// ---------------------------------------------------------------------------
// searchsorted (numpy.searchsorted; the reference has none): for every
// needle of a strided box, how many of the m sorted keys sort strictly before
// it (side 0, left) or not after it (side 1, right), in the canonical order.
// rt_sort_bounds is the W-1 splitter form, one thread a splitter and every
// probe in HBM; this is the kernel for 10^8 needles.
//
// The search, search_count: a lower / upper bound over cnt keys in a FIXED
// number of trips with no branch: `lo` and the remaining length `len` start
// at 0 and cnt; a trip probes key[lo + half - 1], half = len / 2, adds half
// to lo when the probe is on the needle's low side and takes half off len.
// The answer stays in [lo, lo + len]; len reaches 1 after ceil(log2 cnt)
// trips and further trips do nothing (half = 0, the probe is clamped to
// key[lo]), so the host fixes the trip count from the size alone and a wave
// never diverges.  One last probe of key[lo] closes it.
//
// LDS regime, m <= SRCH_LDS_BYTES / key width: every block stages all of v,
// as canonical keys, in 64 KB of LDS (two blocks fit the CU's 160 KB) and
// then grid-strides over the needles; no probe leaves the CU.
// FENCE regime, larger m: with seg = ceil(m / SRCH_FENCE) the block stages
// the G = ceil(m / seg) <= SRCH_FENCE keys v[0], v[seg], v[2 seg], ..; only
// real keys, no padding, so no needle value needs a special case.  A needle
// takes j = search_count(fence) in LDS.  j == 0: v[0] is already on the high
// side, the answer is 0.  Else fence[j-1] = v[(j-1) seg] is on the low side
// and v[j seg], if it exists, is not, so the answer lies in ((j-1) seg,
// j seg] and is (j-1) seg + search_count(v[(j-1) seg .. min(j seg, m))): one
// segment of at most seg keys in global memory, trips fixed by seg.  This
// holds for either side because "low side" is the same predicate in the
// fence and in the segment, and it holds when a run of duplicates spans many
// fence entries: the predicate is monotone over the sorted keys, the fence
// is a subsequence of them, and the fence search returns the boundary of
// the predicate in that subsequence, whichever entries are equal.
//
// Needles are walked as rt_hist walks its box (hist_box_args: 16-byte loads
// under the rt_arg_flat rule, else by element) and the results are written
// dense in C order.
// ---------------------------------------------------------------------------

namespace {

enum {
    SRCH_BLOCK = 256,
    SRCH_FENCE = 4096,
    SRCH_LDS_BYTES = 64 * 1024,
    SRCH_GRID_CAP = 1024                    // 256 CUs x 2 blocks x 2
};

struct SearchArgs {
    HistArgs box;            // the walk of the needles
    int64_t m, seg;          // keys; FENCE: keys per segment, else 0
    int lds_n;               // keys staged in LDS (m, or the fence's G)
    int lds_trips, seg_trips, right;
};

int search_trips(int64_t cnt) {
    int t = 0;
    while (((int64_t)1 << t) < cnt) ++t;
    return t;
}

// CANON: `key` holds canonical keys (LDS), else raw keys (global memory)
template <typename T, bool CANON>
__device__ __forceinline__ int64_t search_count(
    const SortU<T> *key, int64_t cnt, int trips, SortU<T> x, int right) {
    using U = SortU<T>;
    if (cnt == 0) return 0;             // uniform: cnt is the same in a block
    int64_t lo = 0, len = cnt;
    for (int i = 0; i < trips; ++i) {
        const int64_t half = len >> 1;
        const U raw = key[lo + (half ? half - 1 : 0)];
        const U k = CANON ? raw : rt_sort_canon<T>(raw);
        const bool low = k < x || (right && k == x);
        lo += low ? half : 0;
        len -= half;
    }
    const U raw = key[lo];
    const U k = CANON ? raw : rt_sort_canon<T>(raw);
    return lo + ((k < x || (right && k == x)) ? 1 : 0);
}

template <typename T>
__device__ __forceinline__ int64_t search_one(
    const SearchArgs &s, const SortU<T> *lds, const SortU<T> *__restrict__ v,
    SortU<T> needle) {
    const SortU<T> x = rt_sort_canon<T>(needle);
    const int64_t j =
        search_count<T, true>(lds, s.lds_n, s.lds_trips, x, s.right);
    if (s.seg == 0 || j == 0) return j;
    const int64_t s0 = (j - 1) * s.seg;
    const int64_t cnt = s.m - s0 < s.seg ? s.m - s0 : s.seg;
    return s0 + search_count<T, false>(v + s0, cnt, s.seg_trips, x, s.right);
}

template <typename T, typename L>
__global__ __launch_bounds__(256) void search_kernel(
    const SortU<T> *__restrict__ v, const SortU<T> *__restrict__ in,
    SearchArgs s, int64_t *__restrict__ out) {
    using U = SortU<T>;
    extern __shared__ __align__(16) unsigned char search_lds[];
    U *lds = reinterpret_cast<U *>(search_lds);
    const int tid = threadIdx.x;
    const int64_t step = s.seg ? s.seg : 1;
    for (int k = tid; k < s.lds_n; k += 256)
        lds[k] = rt_sort_canon<T>(v[(int64_t)k * step]);
    __syncthreads();

    constexpr int PER = sizeof(L) / sizeof(U);
    const HistArgs &a = s.box;
    const L *src = reinterpret_cast<const L *>(in);
    const int64_t S = (int64_t)gridDim.x * 256;
    for (int64_t u = a.u0 + (int64_t)blockIdx.x * 256 + tid; u < a.u1; u += S) {
        const L unit = src[hist_unit_off(a, u)];
        U e[PER];
        __builtin_memcpy(e, &unit, sizeof(L));
#pragma unroll
        for (int j = 0; j < PER; ++j)
            out[u * PER + j] = search_one<T>(s, lds, v, e[j]);
    }
    const int64_t t = (int64_t)blockIdx.x * 256 + tid;
    if (t < a.tailn)
        out[a.tail0 + t] = search_one<T>(s, lds, v, in[a.tail0 + t]);
}

template <typename T, typename L>
int search_launch(hipStream_t st, const void *v, const void *src,
                  const SearchArgs &s, int64_t nunits, void *out) {
    using U = SortU<T>;
    int64_t blocks = (nunits + 255) / 256;
    if (blocks > SRCH_GRID_CAP) blocks = SRCH_GRID_CAP;
    if (blocks < 1) blocks = 1;             // the scalar tail alone
    hipLaunchKernelGGL((search_kernel<T, L>), dim3((unsigned)blocks),
                       dim3(256), (size_t)s.lds_n * sizeof(U), st,
                       static_cast<const U *>(v), static_cast<const U *>(src),
                       s, static_cast<int64_t *>(out));
    return launched("rt_searchsorted");
}

}  // namespace

extern "C" int rt_searchsorted_geometry(int *block, int *fence,
                                        int64_t *lds_max, int *grid_cap) {
    if (block) *block = SRCH_BLOCK;
    if (fence) *fence = SRCH_FENCE;
    if (lds_max)
        for (int k = 0; k < 4; ++k) lds_max[k] = SRCH_LDS_BYTES >> k;
    if (grid_cap) *grid_cap = SRCH_GRID_CAP;
    return 0;
}

extern "C" int rt_searchsorted(uintptr_t stream, const void *v, int64_t m,
                               const void *x, int64_t x_off, int nd,
                               const int64_t *shape, const int64_t *strides,
                               int dtype, int side, void *out) {
    const char *who = "rt_searchsorted";
    int64_t n;
    if (box_extents(who, nd, 1, shape, strides, strides, &n)) return 1;
    if (dtype < RT_F64 || dtype > RT_U8) return fail(who, "bad dtype");
    if (side != 0 && side != 1) return fail(who, "bad side");
    if (m < 0) return fail(who, "negative m");
    if (m >= (1LL << 40)) return fail(who, "m out of range");
    if (m > 0 && !v) return fail(who, "NULL v");
    if (n == 0) return 0;
    if (!x) return fail(who, "NULL x");
    if (!out) return fail(who, "NULL out");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dtype_dispatch<7>(who, dtype, [&](auto t) {
        using T = decltype(t);
        SearchArgs s;
        int64_t nunits;
        const bool vec = hist_box_args(x, x_off, nd, shape, strides, sizeof(T),
                                       n, &s.box, &nunits);
        s.box.nbins = 0, s.box.regime = 0, s.box.stage_edges = 0;
        s.box.u0 = 0, s.box.u1 = nunits;
        s.m = m, s.right = side;
        if (m <= SRCH_LDS_BYTES / (int64_t)sizeof(T)) {
            s.seg = 0, s.seg_trips = 0;
            s.lds_n = (int)m;
        } else {
            s.seg = (m + SRCH_FENCE - 1) / SRCH_FENCE;
            s.seg_trips = search_trips(s.seg);
            s.lds_n = (int)((m + s.seg - 1) / s.seg);
        }
        s.lds_trips = search_trips(s.lds_n);
        const void *src = static_cast<const T *>(x) + x_off;
        return vec ? search_launch<T, uint4>(st, v, src, s, nunits, out)
                   : search_launch<T, SortU<T>>(st, v, src, s, nunits, out);
    });
}

// ---------------------------------------------------------------------------
// partition / argpartition (numpy.partition, numpy.argpartition; the reference
// has neither): the data movement around keys that rt_select_pass found, one
// stable split of a dense run about P <= PART_NPIV_MAX pivots, distinct
// ascending canonical keys.  The bucket of a key k is
//     b(k) = 2 * (number of pivots < canon(k)) + (canon(k) equals a pivot),
// 2P + 1 buckets: below the first pivot, equal to it, between the first two,
// ..  The output is the buckets in ascending order, each in input order; the
// raw bits are moved.  Three launches, none of which waits for another block,
// no atomics: the output is fixed by the input.
//
// Tiling (count and scatter alike): a tile is PART_BLOCK x PART_KPL consecutive
// keys and lane t owns keys [t * KPL, (t + 1) * KPL) of it, read as KPL *
// sizeof(key) / 16 loads of 16 bytes when the run is 16-byte aligned and the
// tile whole (else key by key, guarded by n).  A block walks a contiguous
// range of tiles.  The buckets of a lane's keys are computed in registers
// (the pivots are kernel arguments, compared in the key's own width) and
// COUNTED IN PACKED WORDS: a word W holds sizeof(W) / 2 fields of 16 bits, one
// per bucket; a lane adds 1 << 16 f for a key of bucket f.  A tile has 4096
// keys, so no field of a lane, wave or tile sum can carry into the next, and
// ONE shuffle scan of a word over the wave is the per-bucket prefix of all
// its fields at once.  The last bucket, 2P, has no field: its counts are what
// is left of the keys.  Word classes: P = 1, the top-k case: one uint32, the
// two fields "below" and "equal", the third bucket derived; P <= 4: two
// uint64; P <= 8: four uint64.
//   part_count_k    per tile the wave's packed totals (the scan's last lane);
//                   lane f of each wave keeps the running 64-bit count of
//                   bucket f.  counts[bucket][block], int64.
//   part_scan_k     one block: base[b][blk] = the keys of lower buckets + the
//                   keys of bucket b in the blocks before; totals[b].
//   part_scatter_k  the same walk recomputes the buckets.  A key of bucket f
//                   goes to: the block's base of f (LDS, advanced tile by
//                   tile) + field f of (the packed totals of the waves below,
//                   a 4-entry LDS table, + the exclusive wave scan + the
//                   lane's earlier keys).  Both LDS tables are double
//                   buffered: one barrier a tile.  Stores are direct, key by
//                   key: a lane's keys of one bucket are consecutive in the
//                   output, and so are those of neighbouring lanes.
// ---------------------------------------------------------------------------

namespace {

enum {
    PART_BLOCK = 256,
    PART_KPL = 16,                          // keys per lane
    PART_TILE = PART_BLOCK * PART_KPL,      // < 2^16: a field holds a tile
    PART_GRID_CAP = 2048,                   // 256 CUs x 8 blocks
    PART_NPIV_MAX = 8,                      // = SELECT_NQ_MAX
    PART_NB_MAX = 2 * PART_NPIV_MAX + 1
};

struct PartPivots {
    uint64_t p[PART_NPIV_MAX];
};

struct PartPlan {
    int64_t ntiles, tpb;
    int nblocks;
};

PartPlan part_plan(int64_t n) {
    PartPlan p;
    p.ntiles = (n + PART_TILE - 1) / PART_TILE;
    p.tpb = (p.ntiles + PART_GRID_CAP - 1) / PART_GRID_CAP;
    if (p.tpb < 1) p.tpb = 1;
    p.nblocks = (int)((p.ntiles + p.tpb - 1) / p.tpb);
    return p;
}

// int64 slots of the scratch: counts[nb][nblocks], base[nb][nblocks],
// totals[nb], nb = 2 npiv + 1
int64_t part_scratch_bytes(int64_t n, int npiv) {
    const PartPlan p = part_plan(n);
    const int64_t nb = 2 * npiv + 1;
    return ((2 * nb * p.nblocks + nb) * 8 + 15) & ~15LL;
}

template <typename W>
__device__ __forceinline__ W part_shfl_up(W v, int off) {
    if constexpr (sizeof(W) == 8)
        return (W)__shfl_up((unsigned long long)v, off);
    else
        return (W)__shfl_up((unsigned)v, off);
}

template <typename W>
__device__ __forceinline__ W part_wave_incl(W x, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const W y = part_shfl_up<W>(x, off);
        if (lane >= off) x += y;
    }
    return x;
}

template <typename W>
__device__ __forceinline__ W part_wave_last(W x) {
    if constexpr (sizeof(W) == 8)
        return (W)__shfl((unsigned long long)x, 63);
    else
        return (W)__shfl((unsigned)x, 63);
}

// one key of bucket f into the packed words; bucket nf (the last) has no field
template <typename W, int NW>
__device__ __forceinline__ void part_add(W *a, int f, int nf) {
    constexpr int FPW = (int)sizeof(W) / 2;
#pragma unroll
    for (int k = 0; k < NW; ++k)
        a[k] += (f < nf && f / FPW == k) ? (W)((W)1 << (16 * (f % FPW)))
                                         : (W)0;
}

// field f < NW * FPW of the packed words
template <typename W, int NW>
__device__ __forceinline__ int part_field(const W *a, int f) {
    constexpr int FPW = (int)sizeof(W) / 2;
    W v = a[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) v = f / FPW == k ? a[k] : v;
    return (int)((v >> (16 * (f % FPW))) & (W)0xffff);
}

// the sum of every field (at most a tile: no carry)
template <typename W, int NW>
__device__ __forceinline__ int part_field_sum(const W *a) {
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) s += a[k];
    s += s >> 32;
    s += s >> 16;
    return (int)(s & 0xffffull);
}

// The lane's KPL raw keys of the tile at `base` (0 past n), their buckets,
// and the packed counts of the lane's valid keys.
template <typename T, typename W, int NW, int PMAX>
__device__ __forceinline__ void part_tile(
    const SortU<T> *__restrict__ keys, int64_t n, int64_t base, int t,
    bool vec, const PartPivots &pv, int npiv, SortU<T> *raw, uint8_t *bk,
    W *w) {
    using U = SortU<T>;
    const int64_t i0 = base + (int64_t)t * PART_KPL;
    if (vec && base + PART_TILE <= n) {
        constexpr int NL = PART_KPL * (int)sizeof(U) / 16;
        const uint4 *src = reinterpret_cast<const uint4 *>(keys + i0);
        uint4 q[NL];
#pragma unroll
        for (int k = 0; k < NL; ++k) q[k] = src[k];
        __builtin_memcpy(raw, q, sizeof(q));
    } else {
#pragma unroll
        for (int j = 0; j < PART_KPL; ++j)
            raw[j] = i0 + j < n ? keys[i0 + j] : (U)0;
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = 0;
#pragma unroll
    for (int j = 0; j < PART_KPL; ++j) {
        const U c = rt_sort_canon<T>(raw[j]);
        int lt = 0, eq = 0;
#pragma unroll
        for (int q = 0; q < PMAX; ++q) {
            const U p = (U)pv.p[q];
            lt += (q < npiv && p < c) ? 1 : 0;
            eq |= (q < npiv && p == c) ? 1 : 0;
        }
        bk[j] = (uint8_t)(2 * lt + eq);
        if (i0 + j < n) part_add<W, NW>(w, bk[j], 2 * npiv);
    }
}

template <typename T, typename W, int NW, int PMAX>
__global__ __launch_bounds__(256) void part_count_k(
    const SortU<T> *__restrict__ keys, int64_t n, int64_t tpb, int64_t ntiles,
    int vec, PartPivots pv, int npiv, int64_t *__restrict__ counts) {
    constexpr int FPW = (int)sizeof(W) / 2;
    __shared__ int64_t wsum[4][2 * PART_NPIV_MAX];
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
    const int nf = 2 * npiv;
    const int64_t tile0 = (int64_t)blockIdx.x * tpb;
    const int64_t tile1 = tile0 + tpb < ntiles ? tile0 + tpb : ntiles;
    int64_t mine = 0;       // lane f < nf: the wave's keys of bucket f
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        SortU<T> raw[PART_KPL];
        uint8_t bk[PART_KPL];
        W w[NW];
        part_tile<T, W, NW, PMAX>(keys, n, tile * PART_TILE, t, vec != 0, pv,
                                  npiv, raw, bk, w);
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const W tot = part_wave_last<W>(part_wave_incl<W>(w[k], lane));
            if (lane / FPW == k)
                mine += (int64_t)((tot >> (16 * (lane % FPW))) & (W)0xffff);
        }
    }
    if (lane < 2 * PART_NPIV_MAX) wsum[wv][lane] = lane < nf ? mine : 0;
    __syncthreads();
    if (t <= nf) {
        int64_t c;
        if (t < nf) {
            c = wsum[0][t] + wsum[1][t] + wsum[2][t] + wsum[3][t];
        } else {            // the last bucket: what is left of the block's keys
            const int64_t lo = tile0 * PART_TILE;
            const int64_t hi = tile1 * PART_TILE < n ? tile1 * PART_TILE : n;
            c = hi - lo;
            for (int f = 0; f < nf; ++f)
                c -= wsum[0][f] + wsum[1][f] + wsum[2][f] + wsum[3][f];
        }
        counts[(int64_t)t * gridDim.x + blockIdx.x] = c;
    }
}

// one block: base[b][blk] = (keys of the buckets below b) + (keys of bucket b
// in the blocks before blk); totals[b] = the keys of bucket b
__global__ __launch_bounds__(256) void part_scan_k(
    const int64_t *__restrict__ counts, int64_t *__restrict__ base,
    int64_t *__restrict__ totals, int nblocks, int nb) {
    __shared__ unsigned long long wsum[2][4];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int per = (nblocks + 255) / 256;
    const int lo = t * per < nblocks ? t * per : nblocks;
    const int hi = lo + per < nblocks ? lo + per : nblocks;
    unsigned long long carry = 0;
    for (int b = 0; b < nb; ++b) {
        const int64_t *row = counts + (int64_t)b * nblocks;
        unsigned long long s = 0;
        for (int i = lo; i < hi; ++i) s += (unsigned long long)row[i];
        const unsigned long long x = sort_wave_incl(s, lane);
        if (lane == 63) wsum[b & 1][w] = x;
        __syncthreads();
        unsigned long long run = carry + x - s, tot = 0;
        for (int k = 0; k < 4; ++k) {
            run += k < w ? wsum[b & 1][k] : 0ull;
            tot += wsum[b & 1][k];
        }
        int64_t *orow = base + (int64_t)b * nblocks;
        for (int i = lo; i < hi; ++i) {
            orow[i] = (int64_t)run;
            run += (unsigned long long)row[i];
        }
        if (t == 0) totals[b] = (int64_t)tot;
        carry += tot;
    }
}

template <typename T, typename W, int NW, int PMAX>
__global__ __launch_bounds__(256) void part_scatter_k(
    const SortU<T> *__restrict__ kin, SortU<T> *__restrict__ kout,
    const int64_t *__restrict__ vin, int64_t *__restrict__ vout, int64_t val0,
    int64_t n, int64_t tpb, int64_t ntiles, int vec, PartPivots pv, int npiv,
    const int64_t *__restrict__ base) {
    __shared__ W wtot[2][4][NW];                // double-buffered: one
    __shared__ int64_t gbase[2][2 * PMAX + 1];  // barrier a tile
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
    const int nf = 2 * npiv;
    if (t <= nf) gbase[0][t] = base[(int64_t)t * gridDim.x + blockIdx.x];
    const int64_t tile0 = (int64_t)blockIdx.x * tpb;
    const int64_t tile1 = tile0 + tpb < ntiles ? tile0 + tpb : ntiles;
    int buf = 0;
    for (int64_t tile = tile0; tile < tile1; ++tile, buf ^= 1) {
        SortU<T> raw[PART_KPL];
        uint8_t bk[PART_KPL];
        W w[NW], before[NW], tt[NW];
        const int64_t tbase = tile * PART_TILE;
        part_tile<T, W, NW, PMAX>(kin, n, tbase, t, vec != 0, pv, npiv, raw,
                                  bk, w);
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const W x = part_wave_incl<W>(w[k], lane);
            before[k] = x - w[k];
            if (lane == 63) wtot[buf][wv][k] = x;
        }
        __syncthreads();        // also orders gbase[buf] before its readers
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            tt[k] = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const W s = wtot[buf][q][k];
                before[k] += q < wv ? s : (W)0;
                tt[k] += s;
            }
        }
        if (t <= nf) {          // the bases of the next tile
            const int64_t left = n - tbase;
            const int nvalid = left < PART_TILE ? (int)left : (int)PART_TILE;
            const int c = t < nf ? part_field<W, NW>(tt, t)
                                 : nvalid - part_field_sum<W, NW>(tt);
            gbase[buf ^ 1][t] = gbase[buf][t] + c;
        }
        const int64_t i0 = tbase + (int64_t)t * PART_KPL;
#pragma unroll
        for (int j = 0; j < PART_KPL; ++j) {
            if (i0 + j < n) {
                const int f = bk[j];
                // the valid keys of a tile are a prefix of it: t * KPL + j of
                // them come before this one
                const int pos =
                    f < nf ? part_field<W, NW>(before, f)
                           : t * PART_KPL + j - part_field_sum<W, NW>(before);
                const int64_t dst = gbase[buf][f] + pos;
                if (kout) kout[dst] = raw[j];
                if (vout) vout[dst] = vin ? vin[i0 + j] : val0 + i0 + j;
                part_add<W, NW>(before, f, nf);
            }
        }
    }
}

template <typename T, typename W, int NW, int PMAX>
int part_launch(hipStream_t st, const void *in, void *out, const void *vals_in,
                int64_t val0, void *vals_out, int64_t n, int npiv,
                const PartPivots &pv, void *scratch) {
    using U = SortU<T>;
    const PartPlan p = part_plan(n);
    const int nb = 2 * npiv + 1;
    int64_t *counts = static_cast<int64_t *>(scratch);
    int64_t *base = counts + (int64_t)nb * p.nblocks;
    int64_t *totals = base + (int64_t)nb * p.nblocks;
    const int vec = reinterpret_cast<uintptr_t>(in) % 16 == 0;
    part_count_k<T, W, NW, PMAX><<<p.nblocks, 256, 0, st>>>(
        static_cast<const U *>(in), n, p.tpb, p.ntiles, vec, pv, npiv, counts);
    part_scan_k<<<1, 256, 0, st>>>(counts, base, totals, p.nblocks, nb);
    part_scatter_k<T, W, NW, PMAX><<<p.nblocks, 256, 0, st>>>(
        static_cast<const U *>(in), static_cast<U *>(out),
        static_cast<const int64_t *>(vals_in),
        static_cast<int64_t *>(vals_out), val0, n, p.tpb, p.ntiles, vec, pv,
        npiv, base);
    return launched("rt_partition");
}

template <typename T>
int part_run(hipStream_t st, const void *in, void *out, const void *vals_in,
             int64_t val0, void *vals_out, int64_t n, int npiv,
             const PartPivots &pv, void *scratch) {
    if (npiv == 1)
        return part_launch<T, uint32_t, 1, 1>(st, in, out, vals_in, val0,
                                              vals_out, n, npiv, pv, scratch);
    if (npiv <= 4)
        return part_launch<T, uint64_t, 2, 4>(st, in, out, vals_in, val0,
                                              vals_out, n, npiv, pv, scratch);
    return part_launch<T, uint64_t, 4, 8>(st, in, out, vals_in, val0,
                                          vals_out, n, npiv, pv, scratch);
}

}  // namespace

extern "C" int rt_partition_geometry(int *block, int *keys_per_lane,
                                     int *grid_cap, int *npiv_max) {
    if (block) *block = PART_BLOCK;
    if (keys_per_lane) *keys_per_lane = PART_KPL;
    if (grid_cap) *grid_cap = PART_GRID_CAP;
    if (npiv_max) *npiv_max = PART_NPIV_MAX;
    return 0;
}

extern "C" int64_t rt_partition_scratch(int64_t n, int npiv) {
    if (n < 0 || n >= (1LL << 40)) return -1;
    if (npiv < 1 || npiv > PART_NPIV_MAX) return -1;
    return part_scratch_bytes(n, npiv);
}

extern "C" int rt_partition(uintptr_t stream, const void *in, void *out,
                            const void *vals_in, int64_t val0, void *vals_out,
                            int64_t n, int dtype, int npiv,
                            const uint64_t *pivots, void *scratch,
                            int64_t scratch_bytes, int64_t *bucket_counts) {
    const char *who = "rt_partition";
    if (dtype < RT_F64 || dtype > RT_U8) return fail(who, "bad dtype");
    if (n < 0) return fail(who, "negative n");
    if (n >= (1LL << 40)) return fail(who, "n out of range");
    if (npiv < 1 || npiv > PART_NPIV_MAX)
        return fail(who, "npiv out of range");
    if (!pivots) return fail(who, "NULL pivots");
    const int width = 8 * dtype_size(dtype);
    PartPivots pv;
    for (int q = 0; q < PART_NPIV_MAX; ++q) pv.p[q] = 0;
    for (int q = 0; q < npiv; ++q) {
        if (width < 64 && (pivots[q] >> width) != 0)
            return fail(who, "pivots: bits above the key width");
        if (q && pivots[q] <= pivots[q - 1])
            return fail(who, "pivots not distinct and ascending");
        pv.p[q] = pivots[q];
    }
    if (n == 0) {
        if (bucket_counts)
            for (int b = 0; b < 2 * npiv + 1; ++b) bucket_counts[b] = 0;
        return 0;
    }
    if (!in) return fail(who, "NULL in");
    if (!out && !vals_out) return fail(who, "NULL out and vals_out");
    if (!scratch) return fail(who, "NULL scratch");
    if (reinterpret_cast<uintptr_t>(scratch) & 15)
        return fail(who, "scratch not 16-byte aligned");
    if (scratch_bytes < part_scratch_bytes(n, npiv))
        return fail(who, "scratch_bytes too small (rt_partition_scratch)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype_dispatch<7>(who, dtype, [&](auto t) {
            return part_run<decltype(t)>(st, in, out, vals_in, val0, vals_out,
                                         n, npiv, pv, scratch);
        }))
        return 1;
    if (!bucket_counts) return 0;
    const PartPlan p = part_plan(n);
    const int nb = 2 * npiv + 1;
    HIP_CHECK(hipMemcpyAsync(
        bucket_counts,
        static_cast<int64_t *>(scratch) + (int64_t)2 * nb * p.nblocks,
        nb * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

// ---------------------------------------------------------------------------
// groupby reductions (the reference's RambaGroupby, ramba.py:10290-10607): a
// keyed reduction of values.  The rows of one axis of a strided box carry a
// group label each; out[.., g, ..] is the reduction over the rows of group g.
// The host hands the labels over as a CSR: `members`, the row numbers stably
// sorted by label, and `seg`, ngroups + 1 offsets into it (both int32).  No
// kernel uses an atomic: every output is combined in an order fixed by the
// shape, the labels and the constants below, so a float result has the same
// bits from run to run.
//
// Accumulators: floats in their own type; SUM / PROD of integers in int64
// with wrap-around; MIN / MAX in the element type (RT_U8 is bool: identities
// 1 and 0); COUNT_VALID, the int64 number of non-NaN members, is a SUM of
// (x == x).  skipna replaces a NaN by the identity.  Float MIN / MAX
// propagate NaN and keep the first of two equal values, as the scalar loops
// of np.minimum.at / np.maximum.at do.
//
// Regimes (rt_group_regime), chosen from the strides:
//   ROWS         another axis has the unit stride (or no axis has).  Lanes
//                lie along that axis (16-byte loads under the rule of
//                rt_arg_flat_regime, else element loads); a block owns one
//                group and a tile of 256 lanes, which is several short rows
//                of the remaining axes when the lane axis is shorter.  The
//                group's member rows are staged through LDS GROUP_MEMBER_TILE
//                at a time as element offsets, and every lane walks them in
//                ascending order, four loads in flight, combining in order:
//                each input byte is read once, and a float SUM equals the
//                sequential np.add.at bit for bit.
//   ROWS_SPLIT   ROWS when ngroups x tiles cannot fill the chip and the axis
//                is long: a member list is cut into chunks of GROUP_CHUNK
//                rows, a block reduces one chunk into a partial, and a second
//                launch combines a group's partials in ascending order.
//   LINE_SELECT  the group axis has the unit stride (1-D included) and
//                ngroups <= GROUP_SELECT_MAX.  A small launch turns the CSR
//                back into one label byte per row.  A block reads a span of a
//                line with its labels, each lane keeps GROUP_SELECT_MAX
//                register accumulators and combines into each the value or
//                the identity (compare-select, no dynamic register index);
//                lanes merge in a shuffle tree, waves through LDS, and a
//                second launch combines the blocks of a line in ascending
//                order.
//   LINE_GATHER  as above with more groups: one wave per (line, chunk of
//                GROUP_GATHER_CHUNK members) gathers x[line, members[j]], j
//                ascending per lane, merges in a shuffle tree; a second
//                launch combines the chunks in order.  Cache lines shared
//                between groups are read once per group.
// Chunk c of group g owns the partial slot seg[g] / chunk + g + c: at most
// K / chunk + ngroups slots, found again from a slot number by a binary
// search on seg.  Member rows and seg offsets are clamped into range before
// use, so a malformed CSR gives wrong numbers, never a wild address.
// ---------------------------------------------------------------------------

namespace {

enum { GROUP_SUM = 0, GROUP_PROD = 1, GROUP_MIN = 2, GROUP_MAX = 3,
       GROUP_COUNT_VALID = 4 };
enum { GROUP_ROWS = 0, GROUP_ROWS_SPLIT = 1, GROUP_LINE_SELECT = 2,
       GROUP_LINE_GATHER = 3 };
enum {
    GROUP_BLOCK = 256,
    GROUP_MEMBER_TILE = 256,      // member rows staged in LDS at a time
    GROUP_CHUNK = 512,            // rows per partial, ROWS_SPLIT
    GROUP_SPLIT_BLOCKS = 1024,    // split below this many (group, tile) pairs
    GROUP_SELECT_MAX = 16,        // register accumulators per lane
    GROUP_SELECT_BLOCKS = 2048,   // blocks of LINE_SELECT, over all lines
    GROUP_GATHER_CHUNK = 1024,    // members per wave, LINE_GATHER
    GROUP_GRID_CAP = 1 << 16      // blocks per launch; work items beyond loop
};

// combining two accumulators of type A under SUM / PROD / MIN / MAX
template <typename A, int OP>
struct GroupAcc {
    static constexpr bool F = std::is_floating_point<A>::value;

    static __host__ __device__ __forceinline__ A identity() {
        if constexpr (OP == GROUP_SUM) {
            return A(0);
        } else if constexpr (OP == GROUP_PROD) {
            return A(1);
        } else if constexpr (F) {
            return OP == GROUP_MIN ? A(__builtin_inf()) : A(-__builtin_inf());
        } else if constexpr (std::is_same<A, uint8_t>::value) {
            return OP == GROUP_MIN ? A(1) : A(0);
        } else {
            return OP == GROUP_MIN ? std::numeric_limits<A>::max()
                                   : std::numeric_limits<A>::min();
        }
    }

    static __device__ __forceinline__ A comb(A a, A b) {
        if constexpr (OP == GROUP_SUM) {
            if constexpr (F) return a + b;
            else return (A)((uint64_t)a + (uint64_t)b);
        } else if constexpr (OP == GROUP_PROD) {
            if constexpr (F) return a * b;
            else return (A)((uint64_t)a * (uint64_t)b);
        } else if constexpr (OP == GROUP_MIN) {
            if constexpr (F) return (a <= b || a != a) ? a : b;
            else return b < a ? b : a;
        } else {
            if constexpr (F) return (a >= b || a != a) ? a : b;
            else return b > a ? b : a;
        }
    }
};

// an element of type T as an accumulator of reduction OP
template <typename T, int OP>
struct GroupRed {
    static constexpr bool F = std::is_floating_point<T>::value;
    static constexpr int AOP = OP == GROUP_COUNT_VALID ? GROUP_SUM : OP;
    using A = std::conditional_t<
        OP == GROUP_COUNT_VALID || (!F && OP <= GROUP_PROD), int64_t, T>;
    using Acc = GroupAcc<A, AOP>;

    static __device__ __forceinline__ A lift(T x, int skipna) {
        if constexpr (OP == GROUP_COUNT_VALID) {
            if constexpr (F) return (A)(x == x);
            else return A(1);
        } else {
            if constexpr (F)
                if (skipna && x != x) return Acc::identity();
            return (A)x;
        }
    }
};

struct GroupArgs {
    int64_t K, sK, osG;      // group axis: rows, input and output stride
    int64_t ext[3], str[3], ostr[3];   // the other axes, slowest first; in
                                       // ROWS [2] is the lane axis
    int64_t P;               // ext[0] * ext[1] * ext[2]
    int64_t ngroups;
    int64_t items;           // work items of the launch
    int64_t nslots;          // ROWS_SPLIT / LINE_GATHER: partial slots
    int64_t nu, tiles_in, tiles;   // ROWS: lane-axis units, tiles along the
                                   // lane axis, tiles per group
    int64_t bpl, span;       // LINE_SELECT: blocks per line, rows per block
    int lpr_shift;           // ROWS: a block is (256 >> s) rows of (1 << s)
    int split, skipna;
};

// how a second launch finds the partials of output (g, p):
// part[(base + c) * slot_stride + p * p_stride + g * g_stride], c ascending
struct GroupFinArgs {
    int64_t chunk;           // > 0: base and count from seg (slot scheme)
    int64_t count;           // chunk == 0: a fixed count, base 0
    int64_t slot_stride, p_stride, g_stride;
};

__device__ __forceinline__ int64_t group_seg(const int32_t *seg, int64_t g,
                                             int64_t K) {
    const int64_t s = seg[g];
    return s < 0 ? 0 : s > K ? K : s;
}

__device__ __forceinline__ int64_t group_member(const int32_t *members,
                                                int64_t j, int64_t K) {
    const int64_t m = members[j];
    return m < 0 ? 0 : m >= K ? K - 1 : m;
}

// Slot s -> its group g and member range [m0, m1); false for a slot that no
// chunk owns.  base(g) = seg[g] / chunk + g grows strictly with g and
// base(0) = 0, so the owner is the last g with base(g) <= s.
__device__ __forceinline__ bool group_slot(const int32_t *seg,
                                           int64_t ngroups, int64_t K,
                                           int64_t chunk, int64_t s,
                                           int64_t &g, int64_t &m0,
                                           int64_t &m1) {
    int64_t lo = 0, hi = ngroups - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (group_seg(seg, mid, K) / chunk + mid <= s)
            lo = mid;
        else
            hi = mid - 1;
    }
    g = lo;
    const int64_t s0 = group_seg(seg, g, K), s1 = group_seg(seg, g + 1, K);
    const int64_t c = s - (s0 / chunk + g);
    m0 = s0 + c * chunk;
    if (c < 0 || m0 >= s1) return false;
    m1 = m0 + chunk < s1 ? m0 + chunk : s1;
    return true;
}

// position p of the three non-group axes -> input and output offsets
__device__ __forceinline__ void group_line_off(const GroupArgs &a, int64_t p,
                                               int64_t &in_off,
                                               int64_t &out_off) {
    const int64_t q = p / a.ext[2], i2 = p - q * a.ext[2];
    const int64_t i0 = q / a.ext[1], i1 = q - i0 * a.ext[1];
    in_off = i0 * a.str[0] + i1 * a.str[1] + i2 * a.str[2];
    out_off = i0 * a.ostr[0] + i1 * a.ostr[1] + i2 * a.ostr[2];
}

template <typename A>
__device__ __forceinline__ A group_shfl_down(A v, int d) {
    if constexpr (sizeof(A) == 8) {
        uint32_t w[2];
        __builtin_memcpy(w, &v, 8);
        w[0] = __shfl_down(w[0], d);
        w[1] = __shfl_down(w[1], d);
        __builtin_memcpy(&v, w, 8);
        return v;
    } else if constexpr (sizeof(A) == 4) {
        uint32_t w;
        __builtin_memcpy(&w, &v, 4);
        w = __shfl_down(w, d);
        __builtin_memcpy(&v, &w, 4);
        return v;
    } else {
        return (A)__shfl_down((int)v, d);
    }
}

// lane 0 ends with the wave's 64 values combined in a fixed binary tree
template <typename Acc, typename A>
__device__ __forceinline__ A group_wave_tree(A v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v = Acc::comb(v, group_shfl_down<A>(v, d));
    return v;
}

// one load unit (uint4 of 16 / sizeof(T) elements, or one element) combined
// into the lane's accumulators, element by element
template <typename T, int OP, typename L>
__device__ __forceinline__ void group_rows_add(
    typename GroupRed<T, OP>::A *acc, const L &unit, int skipna) {
    using R = GroupRed<T, OP>;
    constexpr int V = sizeof(L) / sizeof(T);
    T e[V];
    __builtin_memcpy(e, &unit, sizeof(L));
#pragma unroll
    for (int i = 0; i < V; ++i)
        acc[i] = R::Acc::comb(acc[i], R::lift(e[i], skipna));
}

template <typename T, int OP, bool VEC>
__global__ __launch_bounds__(256) GEMM_NO_PK_F32 void group_rows_kernel(
    const T *__restrict__ in, GroupArgs a,
    const int32_t *__restrict__ members, const int32_t *__restrict__ seg,
    typename GroupRed<T, OP>::A *__restrict__ out,
    typename GroupRed<T, OP>::A *__restrict__ part) {
    using R = GroupRed<T, OP>;
    using A = typename R::A;
    using L = std::conditional_t<VEC, uint4, T>;
    constexpr int V = sizeof(L) / sizeof(T);
    __shared__ int64_t goff[GROUP_MEMBER_TILE];
    const int tid = threadIdx.x;
    const int64_t u_in = tid & ((1 << a.lpr_shift) - 1);
    const int64_t r_in = tid >> a.lpr_shift;
    const int64_t nouter = a.ext[0] * a.ext[1];

    for (int64_t w = blockIdx.x; w < a.items; w += gridDim.x) {
        const int64_t s = w / a.tiles, t = w - s * a.tiles;
        int64_t g = s, m0, m1;
        if (a.split) {
            if (!group_slot(seg, a.ngroups, a.K, GROUP_CHUNK, s, g, m0, m1))
                continue;                       // the whole block, no barrier
        } else {
            m0 = group_seg(seg, g, a.K);
            m1 = group_seg(seg, g + 1, a.K);
        }
        const int64_t to = t / a.tiles_in, ti = t - to * a.tiles_in;
        const int64_t iu = (ti << a.lpr_shift) + u_in;
        const int64_t o = (to << (8 - a.lpr_shift)) + r_in;
        const bool live = iu < a.nu && o < nouter;
        const int64_t i0 = o / a.ext[1], i1 = o - i0 * a.ext[1];
        const T *base = in + i0 * a.str[0] + i1 * a.str[1]
                        + iu * V * a.str[2];
        A acc[V];
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] = R::Acc::identity();

        for (int64_t tm = m0; tm < m1; tm += GROUP_MEMBER_TILE) {
            const int n = (int)(m1 - tm < GROUP_MEMBER_TILE
                                    ? m1 - tm : GROUP_MEMBER_TILE);
            __syncthreads();                    // the last tile is used up
            for (int j = tid; j < n; j += GROUP_BLOCK)
                goff[j] = group_member(members, tm + j, a.K) * a.sK;
            __syncthreads();
            if (live) {
                int j = 0;
                for (; j + 4 <= n; j += 4) {
                    const L x0 = *reinterpret_cast<const L *>(base + goff[j]);
                    const L x1 =
                        *reinterpret_cast<const L *>(base + goff[j + 1]);
                    const L x2 =
                        *reinterpret_cast<const L *>(base + goff[j + 2]);
                    const L x3 =
                        *reinterpret_cast<const L *>(base + goff[j + 3]);
                    group_rows_add<T, OP, L>(acc, x0, a.skipna);
                    group_rows_add<T, OP, L>(acc, x1, a.skipna);
                    group_rows_add<T, OP, L>(acc, x2, a.skipna);
                    group_rows_add<T, OP, L>(acc, x3, a.skipna);
                }
                for (; j < n; ++j) {
                    const L x0 = *reinterpret_cast<const L *>(base + goff[j]);
                    group_rows_add<T, OP, L>(acc, x0, a.skipna);
                }
            }
        }
        if (!live) continue;                    // no barrier below
        if (a.split) {
            A *p = part + s * a.P + o * a.ext[2] + iu * V;
#pragma unroll
            for (int i = 0; i < V; ++i) p[i] = acc[i];
        } else {
            A *p = out + g * a.osG + i0 * a.ostr[0] + i1 * a.ostr[1]
                   + iu * V * a.ostr[2];
#pragma unroll
            for (int i = 0; i < V; ++i) p[i * a.ostr[2]] = acc[i];
        }
    }
}

// LINE_SELECT, launch 1: label byte of every row from the CSR
__global__ __launch_bounds__(256) void group_labels_kernel(
    const int32_t *__restrict__ members, const int32_t *__restrict__ seg,
    int64_t K, int ngroups, uint8_t *__restrict__ lab) {
    const int64_t S = (int64_t)gridDim.x * GROUP_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x; j < K;
         j += S) {
        int g = 0;      // the last group whose segment starts at or before j
        for (int q = 1; q < ngroups; ++q) g += group_seg(seg, q, K) <= j;
        lab[group_member(members, j, K)] = (uint8_t)g;
    }
}

template <typename T, int OP>
__device__ __forceinline__ void group_select_add(
    typename GroupRed<T, OP>::A *acc, T x, int label, int skipna) {
    using R = GroupRed<T, OP>;
    const typename R::A v = R::lift(x, skipna);
#pragma unroll
    for (int g = 0; g < GROUP_SELECT_MAX; ++g)
        acc[g] = R::Acc::comb(acc[g], label == g ? v : R::Acc::identity());
}

template <typename T, int OP, bool VEC>
__global__ __launch_bounds__(256) GEMM_NO_PK_F32 void group_select_kernel(
    const T *__restrict__ in, GroupArgs a, const uint8_t *__restrict__ lab,
    typename GroupRed<T, OP>::A *__restrict__ part) {
    using R = GroupRed<T, OP>;
    using A = typename R::A;
    using L = std::conditional_t<VEC, uint4, T>;
    constexpr int V = sizeof(L) / sizeof(T);
    constexpr int NG = GROUP_SELECT_MAX;
    __shared__ A wave_acc[GROUP_BLOCK / 64][NG];
    const int tid = threadIdx.x;

    for (int64_t w = blockIdx.x; w < a.items; w += gridDim.x) {
        const int64_t line = w / a.bpl, b = w - line * a.bpl;
        int64_t in_off, out_off;
        group_line_off(a, line, in_off, out_off);
        const T *base = in + in_off;
        const int64_t k0 = b * a.span;
        const int64_t k1 = k0 + a.span < a.K ? k0 + a.span : a.K;
        A acc[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = R::Acc::identity();

        // whole units of [k0, k1); span is a multiple of 256 x 16 bytes
#pragma unroll 2
        for (int64_t u = k0 / V + tid; u < k1 / V; u += GROUP_BLOCK) {
            const L unit = *reinterpret_cast<const L *>(base + u * V * a.sK);
            T e[V];
            uint8_t l[V];
            __builtin_memcpy(e, &unit, sizeof(L));
            __builtin_memcpy(l, __builtin_assume_aligned(lab + u * V, V), V);
#pragma unroll
            for (int i = 0; i < V; ++i)
                group_select_add<T, OP>(acc, e[i], l[i], a.skipna);
        }
        if (VEC && k1 == a.K) {         // the rows past the line's last unit
            const int64_t k = a.K / V * V + tid;
            if (k >= k0 && k < a.K)
                group_select_add<T, OP>(acc, base[k * a.sK], lab[k],
                                        a.skipna);
        }

#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g < a.ngroups) {
                const A v = group_wave_tree<typename R::Acc, A>(acc[g]);
                if ((tid & 63) == 0) wave_acc[tid >> 6][g] = v;
            }
        }
        __syncthreads();
        if (tid < a.ngroups) {
            A v = wave_acc[0][tid];
#pragma unroll
            for (int q = 1; q < GROUP_BLOCK / 64; ++q)
                v = R::Acc::comb(v, wave_acc[q][tid]);
            part[w * a.ngroups + tid] = v;
        }
        __syncthreads();
    }
}

template <typename T, int OP>
__global__ __launch_bounds__(256) GEMM_NO_PK_F32 void group_gather_kernel(
    const T *__restrict__ in, GroupArgs a,
    const int32_t *__restrict__ members, const int32_t *__restrict__ seg,
    typename GroupRed<T, OP>::A *__restrict__ part) {
    using R = GroupRed<T, OP>;
    using A = typename R::A;
    const int lane = threadIdx.x & 63;
    constexpr int WAVES = GROUP_BLOCK / 64;
    for (int64_t w = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
         w < a.items; w += (int64_t)gridDim.x * WAVES) {
        const int64_t line = w / a.nslots, s = w - line * a.nslots;
        int64_t g, m0, m1;
        if (!group_slot(seg, a.ngroups, a.K, GROUP_GATHER_CHUNK, s, g, m0,
                        m1))
            continue;                           // the whole wave
        int64_t in_off, out_off;
        group_line_off(a, line, in_off, out_off);
        const T *base = in + in_off;
        A acc = R::Acc::identity();
#pragma unroll 4
        for (int64_t j = m0 + lane; j < m1; j += 64)
            acc = R::Acc::comb(
                acc, R::lift(base[group_member(members, j, a.K) * a.sK],
                             a.skipna));
        acc = group_wave_tree<typename R::Acc, A>(acc);
        if (lane == 0) part[w] = acc;
    }
}

// the second launch of ROWS_SPLIT, LINE_SELECT and LINE_GATHER: one thread
// per output combines its partials in ascending order
template <typename A, int OP>
__global__ __launch_bounds__(256) GEMM_NO_PK_F32 void group_finish_kernel(
    const A *__restrict__ part, GroupArgs a, GroupFinArgs f,
    const int32_t *__restrict__ seg, A *__restrict__ out) {
    using Acc = GroupAcc<A, OP>;
    const int64_t n = a.ngroups * a.P;
    const int64_t S = (int64_t)gridDim.x * GROUP_BLOCK;
    for (int64_t e = (int64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x; e < n;
         e += S) {
        const int64_t g = e / a.P, p = e - g * a.P;
        int64_t base = 0, count = f.count;
        if (f.chunk) {
            const int64_t s0 = group_seg(seg, g, a.K);
            const int64_t s1 = group_seg(seg, g + 1, a.K);
            base = s0 / f.chunk + g;
            count = s1 > s0 ? (s1 - s0 + f.chunk - 1) / f.chunk : 0;
        }
        const A *src = part + base * f.slot_stride + p * f.p_stride
                       + g * f.g_stride;
        A acc = Acc::identity();
        for (int64_t c = 0; c < count; ++c)
            acc = Acc::comb(acc, src[c * f.slot_stride]);
        int64_t in_off, out_off;
        group_line_off(a, p, in_off, out_off);
        out[g * a.osG + out_off] = acc;
    }
}

// rt_dtype of the accumulator (and of `out`) for an input dtype and op
int group_acc_dtype(int dtype, int op) {
    if (op == GROUP_COUNT_VALID) return RT_I64;
    if (op == GROUP_MIN || op == GROUP_MAX) return dtype;
    return dtype == RT_F64 || dtype == RT_F32 ? dtype : RT_I64;
}

struct GroupPlan {
    int regime;
    GroupArgs a;
    bool vec_ok;             // strides and extents allow 16-byte loads
    int64_t part_bytes;      // partials at the start of the scratch
    int64_t scratch_bytes;   // partials, then LINE_SELECT's label bytes
};

int64_t group_abs(int64_t v) { return v < 0 ? -v : v; }
int64_t group_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Regime, axis roles and launch geometry from the shape and strides alone
// (no pointer, no label): what rt_group_regime and rt_group_scratch report
// is what rt_group_reduce runs.  Arguments are validated by the callers.
void group_plan(int nd, const int64_t *shape, const int64_t *strides,
                const int64_t *out_strides, int axis, int dtype, int op,
                int64_t ngroups, GroupPlan *plan) {
    GroupArgs &a = plan->a;
    const int es = dtype_size(dtype);
    const int64_t V = 16 / es;
    a.K = shape[axis];
    a.sK = strides[axis];
    a.osG = out_strides ? out_strides[axis] : 0;
    a.ngroups = ngroups;
    a.nslots = a.nu = a.tiles_in = a.tiles = a.bpl = a.span = 0;
    a.lpr_shift = a.split = a.skipna = 0;

    // the lane axis of ROWS: the last other axis of unit stride; the group
    // axis takes the lanes (LINE_*) when it alone has the unit stride, or
    // when there is no other axis to take them
    int lane = -1, others = 0, fallback = -1;
    for (int d = 0; d < nd; ++d) {
        if (d == axis || shape[d] == 1) continue;
        ++others;
        if (group_abs(strides[d]) == 1) lane = d;
        if (strides[d] != 0
            && (fallback < 0 || group_abs(strides[d])
                                    <= group_abs(strides[fallback])))
            fallback = d;
    }
    bool line = others == 0;
    if (!line && lane < 0) {
        if (group_abs(a.sK) == 1)
            line = true;
        else
            lane = fallback;
    }
    if (!line && lane < 0)      // every other axis is a broadcast
        for (int d = 0; d < nd; ++d)
            if (d != axis && shape[d] != 1) lane = d;

    // the other axes, right-aligned, the lane axis last
    for (int d = 0; d < 3; ++d) {
        a.ext[d] = 1;
        a.str[d] = a.ostr[d] = 0;
    }
    int k = 2;
    auto place = [&](int d) {
        a.ext[k] = shape[d];
        a.str[k] = strides[d];
        a.ostr[k] = out_strides ? out_strides[d] : 0;
        --k;
    };
    if (!line) place(lane);
    for (int d = nd - 1; d >= 0; --d)
        if (d != axis && (line || d != lane)) place(d);
    if (!line) {
        // fold an axis that is dense over the lane axis, in and out, into it
        while (a.ext[1] > 1 && a.str[1] == a.ext[2] * a.str[2]
               && a.ostr[1] == a.ext[2] * a.ostr[2]) {
            a.ext[2] *= a.ext[1];
            a.ext[1] = a.ext[0];
            a.str[1] = a.str[0];
            a.ostr[1] = a.ostr[0];
            a.ext[0] = 1;
            a.str[0] = a.ostr[0] = 0;
        }
    }
    a.P = a.ext[0] * a.ext[1] * a.ext[2];
    const int64_t asz = dtype_size(group_acc_dtype(dtype, op));

    plan->part_bytes = 0;
    int64_t label_bytes = 0;
    if (!line) {
        plan->vec_ok = a.str[2] == 1 && a.ext[2] % V == 0 && a.sK % V == 0
                       && a.str[0] % V == 0 && a.str[1] % V == 0;
        a.split = ngroups * group_cdiv(a.P, GROUP_BLOCK) < GROUP_SPLIT_BLOCKS
                  && a.K >= 2 * GROUP_CHUNK + 1;
        plan->regime = a.split ? GROUP_ROWS_SPLIT : GROUP_ROWS;
        if (a.split) {
            a.nslots = a.K / GROUP_CHUNK + ngroups;
            plan->part_bytes = a.nslots * a.P * asz;
        }
    } else if (ngroups <= GROUP_SELECT_MAX) {
        plan->regime = GROUP_LINE_SELECT;
        plan->vec_ok = a.sK == 1 && a.K >= V && a.str[0] % V == 0
                       && a.str[1] % V == 0 && a.str[2] % V == 0;
        const int64_t tile = GROUP_BLOCK * V;
        int64_t bpl = GROUP_SELECT_BLOCKS / a.P;
        if (bpl < 1) bpl = 1;
        if (bpl > group_cdiv(a.K, tile)) bpl = group_cdiv(a.K, tile);
        a.span = group_cdiv(group_cdiv(a.K, bpl), tile) * tile;
        a.bpl = group_cdiv(a.K, a.span);
        a.items = a.P * a.bpl;
        plan->part_bytes = (a.items * ngroups * asz + 15) & ~(int64_t)15;
        label_bytes = a.K;
    } else {
        plan->regime = GROUP_LINE_GATHER;
        plan->vec_ok = false;
        a.nslots = a.K / GROUP_GATHER_CHUNK + ngroups;
        a.items = a.P * a.nslots;
        plan->part_bytes = a.items * asz;
    }
    plan->scratch_bytes = plan->part_bytes + label_bytes;
}

// ROWS launch geometry, once the load width is known
void group_rows_geometry(GroupArgs *a, int64_t V) {
    a->nu = a->ext[2] / V;
    int s = 0;
    while (s < 8 && (1LL << s) < a->nu) ++s;
    a->lpr_shift = s;
    a->tiles_in = group_cdiv(a->nu, 1LL << s);
    a->tiles = a->tiles_in * group_cdiv(a->ext[0] * a->ext[1], 256 >> s);
    a->items = (a->split ? a->nslots : a->ngroups) * a->tiles;
}

unsigned group_grid(int64_t blocks) {
    return (unsigned)(blocks < 1 ? 1
                      : blocks > GROUP_GRID_CAP ? GROUP_GRID_CAP : blocks);
}

template <typename A>
int group_finish(hipStream_t st, int aop, const void *part,
                 const GroupArgs &a, const GroupFinArgs &f, const void *seg,
                 void *out) {
    const unsigned grid =
        group_grid(group_cdiv(a.ngroups * a.P, GROUP_BLOCK));
#define GROUP_FIN(OP)                                                      \
    hipLaunchKernelGGL((group_finish_kernel<A, OP>), dim3(grid),           \
                       dim3(GROUP_BLOCK), 0, st,                           \
                       static_cast<const A *>(part), a, f,                 \
                       static_cast<const int32_t *>(seg),                  \
                       static_cast<A *>(out))
    if constexpr (std::is_floating_point<A>::value
                  || std::is_same<A, int64_t>::value) {
        if (aop == GROUP_SUM) GROUP_FIN(GROUP_SUM);
        if (aop == GROUP_PROD) GROUP_FIN(GROUP_PROD);
    }
    if (aop == GROUP_MIN) GROUP_FIN(GROUP_MIN);
    if (aop == GROUP_MAX) GROUP_FIN(GROUP_MAX);
#undef GROUP_FIN
    return launched("rt_group_reduce (combine)");
}

template <typename T, int OP>
int group_run(hipStream_t st, const T *src, bool aligned, GroupPlan &plan,
              const int32_t *members, const int32_t *seg, void *out,
              void *scratch) {
    using R = GroupRed<T, OP>;
    using A = typename R::A;
    GroupArgs &a = plan.a;
    A *part = static_cast<A *>(scratch);
    A *outp = static_cast<A *>(out);
    const bool vec = plan.vec_ok && aligned;
    GroupFinArgs f = {0, 0, 0, 0, 0};

    if (plan.regime <= GROUP_ROWS_SPLIT) {
        group_rows_geometry(&a, vec ? 16 / (int64_t)sizeof(T) : 1);
        const unsigned grid = group_grid(a.items);
        if (vec)
            hipLaunchKernelGGL((group_rows_kernel<T, OP, true>), dim3(grid),
                               dim3(GROUP_BLOCK), 0, st, src, a, members,
                               seg, outp, part);
        else
            hipLaunchKernelGGL((group_rows_kernel<T, OP, false>), dim3(grid),
                               dim3(GROUP_BLOCK), 0, st, src, a, members,
                               seg, outp, part);
        if (launched("rt_group_reduce (rows)")) return 1;
        if (!a.split) return 0;
        f.chunk = GROUP_CHUNK;
        f.slot_stride = a.P;
        f.p_stride = 1;
    } else if (plan.regime == GROUP_LINE_SELECT) {
        uint8_t *lab = static_cast<uint8_t *>(scratch) + plan.part_bytes;
        hipLaunchKernelGGL(group_labels_kernel,
                           dim3(group_grid(group_cdiv(a.K, GROUP_BLOCK))),
                           dim3(GROUP_BLOCK), 0, st, members, seg, a.K,
                           (int)a.ngroups, lab);
        if (launched("rt_group_reduce (labels)")) return 1;
        const unsigned grid = group_grid(a.items);
        if (vec)
            hipLaunchKernelGGL((group_select_kernel<T, OP, true>),
                               dim3(grid), dim3(GROUP_BLOCK), 0, st, src, a,
                               lab, part);
        else
            hipLaunchKernelGGL((group_select_kernel<T, OP, false>),
                               dim3(grid), dim3(GROUP_BLOCK), 0, st, src, a,
                               lab, part);
        if (launched("rt_group_reduce (select)")) return 1;
        f.count = a.bpl;
        f.slot_stride = a.ngroups;
        f.p_stride = a.bpl * a.ngroups;
        f.g_stride = 1;
    } else {
        hipLaunchKernelGGL((group_gather_kernel<T, OP>),
                           dim3(group_grid(group_cdiv(a.items, 4))),
                           dim3(GROUP_BLOCK), 0, st, src, a, members, seg,
                           part);
        if (launched("rt_group_reduce (gather)")) return 1;
        f.chunk = GROUP_GATHER_CHUNK;
        f.slot_stride = 1;
        f.p_stride = a.nslots;
    }
    return group_finish<A>(st, R::AOP, part, a, f, seg, out);
}

// the checks shared by the four entry points; *n_out = elements of the box
int group_validate(const char *who, int nd, const int64_t *shape,
                   const int64_t *strides, const int64_t *out_strides,
                   int axis, int dtype, int op, int64_t ngroups,
                   int64_t *n_out) {
    if (box_extents(who, nd, 1, shape, strides, out_strides, n_out)) return 1;
    if (axis < 0 || axis >= nd) return fail(who, "axis out of range");
    if (dtype < RT_F64 || dtype > RT_U8) return fail(who, "bad dtype");
    if (op < GROUP_SUM || op > GROUP_COUNT_VALID) return fail(who, "bad op");
    if (ngroups < 1) return fail(who, "ngroups < 1");
    if (ngroups >= (1LL << 31)) return fail(who, "ngroups out of range");
    if (shape[axis] >= (1LL << 31))
        return fail(who, "group axis too long for int32 members");
    if (shape[axis] && *n_out / shape[axis] > (1LL << 46) / ngroups)
        return fail(who, "result too large (ngroups x other extents)");
    return 0;
}

}  // namespace

extern "C" int rt_group_geometry(int *block, int *member_tile, int *chunk,
                                 int *split_blocks, int *select_max,
                                 int *select_blocks, int *gather_chunk,
                                 int *grid_cap) {
    if (block) *block = GROUP_BLOCK;
    if (member_tile) *member_tile = GROUP_MEMBER_TILE;
    if (chunk) *chunk = GROUP_CHUNK;
    if (split_blocks) *split_blocks = GROUP_SPLIT_BLOCKS;
    if (select_max) *select_max = GROUP_SELECT_MAX;
    if (select_blocks) *select_blocks = GROUP_SELECT_BLOCKS;
    if (gather_chunk) *gather_chunk = GROUP_GATHER_CHUNK;
    if (grid_cap) *grid_cap = GROUP_GRID_CAP;
    return 0;
}

extern "C" int rt_group_regime(int nd, const int64_t *shape,
                               const int64_t *strides, int axis, int dtype,
                               int64_t ngroups) {
    int64_t n;
    if (group_validate("rt_group_regime", nd, shape, strides, strides, axis,
                       dtype, GROUP_SUM, ngroups, &n))
        return -1;
    GroupPlan plan;
    group_plan(nd, shape, strides, nullptr, axis, dtype, GROUP_SUM, ngroups,
               &plan);
    return plan.regime;
}

extern "C" int64_t rt_group_scratch(int nd, const int64_t *shape,
                                    const int64_t *strides, int axis,
                                    int dtype, int op, int64_t ngroups) {
    int64_t n;
    if (group_validate("rt_group_scratch", nd, shape, strides, strides, axis,
                       dtype, op, ngroups, &n))
        return -1;
    if (n == 0) return 0;
    GroupPlan plan;
    group_plan(nd, shape, strides, nullptr, axis, dtype, op, ngroups, &plan);
    return plan.scratch_bytes;
}

extern "C" int rt_group_reduce(uintptr_t stream, const void *in,
                               int64_t in_off, int nd, const int64_t *shape,
                               const int64_t *strides, int axis, int dtype,
                               int op, int skipna, const void *members,
                               const void *seg, int64_t ngroups, void *out,
                               const int64_t *out_strides, void *scratch) {
    const char *who = "rt_group_reduce";
    int64_t n;
    if (group_validate(who, nd, shape, strides, out_strides, axis, dtype, op,
                       ngroups, &n))
        return 1;
    if (n == 0) return 0;
    if (!in) return fail(who, "NULL in");
    if (!members) return fail(who, "NULL members");
    if (!seg) return fail(who, "NULL seg");
    if (!out) return fail(who, "NULL out");
    GroupPlan plan;
    group_plan(nd, shape, strides, out_strides, axis, dtype, op, ngroups,
               &plan);
    plan.a.skipna = skipna != 0;
    if (plan.scratch_bytes && !scratch) return fail(who, "NULL scratch");
    if (reinterpret_cast<uintptr_t>(scratch) & 15)
        return fail(who, "scratch not 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int32_t *mem = static_cast<const int32_t *>(members);
    const int32_t *sg = static_cast<const int32_t *>(seg);

    return dtype_dispatch<7>(who, dtype, [&](auto t) {
        using T = decltype(t);
        const T *src = static_cast<const T *>(in) + in_off;
        const bool aligned = reinterpret_cast<uintptr_t>(src) % 16 == 0;
        switch (op) {
            case GROUP_SUM:
                return group_run<T, GROUP_SUM>(st, src, aligned, plan, mem,
                                               sg, out, scratch);
            case GROUP_PROD:
                return group_run<T, GROUP_PROD>(st, src, aligned, plan, mem,
                                                sg, out, scratch);
            case GROUP_MIN:
                return group_run<T, GROUP_MIN>(st, src, aligned, plan, mem,
                                               sg, out, scratch);
            case GROUP_MAX:
                return group_run<T, GROUP_MAX>(st, src, aligned, plan, mem,
                                               sg, out, scratch);
        }
        return group_run<T, GROUP_COUNT_VALID>(st, src, aligned, plan, mem,
                                               sg, out, scratch);
    });
}
