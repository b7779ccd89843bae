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
#include <mutex>
#include <string>
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
