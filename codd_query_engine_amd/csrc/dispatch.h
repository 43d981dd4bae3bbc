// dispatch.h — an implementation part of codd_knn.hip, included there exactly once; not a stand-alone interface.
// ---- kernel dispatch -------------------------------------------------------------------------
// Each run-time choice of a template argument is made in one place: a with_* helper calls the generic lambda `f` with a
// std::integral_constant of the chosen value (usable as a template argument inside f) and returns what f returns (a
// CODD_KNN_* code).  A value no kernel is built for is an error.
#pragma once

namespace {

template <int V>
using IntC = std::integral_constant<int, V>;

// f(IntC<V>) for the V of Vs that equals v, else EINVAL with `unsupported` (a fail() format)
template <int... Vs, typename F>
int with_int(int v, const char* unsupported, F&& f) {
    bool found = false;
    int rc = CODD_KNN_OK;
    ((v == Vs ? (found = true, rc = f(IntC<Vs>{})) : 0), ...);
    return found ? rc : fail(CODD_KNN_EINVAL, unsupported);
}

template <typename F>
int with_dtype(int dtype, F&& f) {
    return with_int<DT_F32, DT_BF16, DT_F16>(dtype, "unknown dtype%s", f);
}

// the NITER values the wide forms serve: rows of 5 .. 16 chunks per lane (f32: 1,025 .. 4,096 elements; 2-byte: 2,049 .. 4,096)
constexpr int kMaxNiter = 16;

// 1 .. 4 chunks per lane: NITER itself; 5 .. kMaxNiter: the wide form (kWideRows); wider: ENOTSUP with `too_wide`
template <typename F>
int with_niter(int niter, const char* too_wide, F&& f) {
    switch (niter) {
        case 1: return f(IntC<1>{});
        case 2: return f(IntC<2>{});
        case 3: return f(IntC<3>{});
        case 4: return f(IntC<4>{});
    }
    if (niter > 4 && niter <= kMaxNiter) return f(IntC<kWideRows>{});
    return fail(CODD_KNN_ENOTSUP, too_wide);
}

// list slots per lane of a top-k list: one for k <= 64, else two
template <typename F>
int with_slots(int k, F&& f) {
    return k <= 64 ? f(IntC<1>{}) : f(IntC<2>{});
}

// 32-query blocks of a filter pass
template <typename F>
int with_nbq(int nbq, F&& f) {
    return with_int<1, 2, 4, 8>(nbq, "bad query block count%s", f);
}

// f(DT, NITER, SLOTS): the form of an exact-score row kernel for the index's rows and k
template <typename F>
int with_row_form(const codd_knn_index* ix, int k, const char* too_wide, F&& f) {
    return with_dtype(ix->dtype, [&](auto dt) {
        return with_niter(niter_of(shape_of(ix)), too_wide, [&](auto ni) {
            return with_slots(k, [&](auto sl) { return f(dt, ni, sl); });
        });
    });
}

// Dynamic LDS above 64 KiB needs the instantiation's opt-in, once per device (the caller's DeviceGuard has made the index's
// device current).  `bytes` must be at least what any launch of `Kernel` asks for.
template <auto Kernel>
int opt_in_lds(size_t bytes) {
    static std::atomic<uint64_t> done{0};  // one bit per device
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const uint64_t bit = dev < 64 ? 1ull << dev : 0ull;
    if (!bit || !(done.load(std::memory_order_acquire) & bit)) {
        HIP_TRY(hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        done.fetch_or(bit, std::memory_order_acq_rel);
    }
    return CODD_KNN_OK;
}

// dynamic LDS of a launch, and what its kernel opts in to when that is above 64 KiB (by default the same: a kernel launched
// with one size only)
struct Lds {
    size_t bytes, opt_in;
    Lds(size_t b) : bytes(b), opt_in(b) {}
    Lds(size_t b, size_t most) : bytes(b), opt_in(most) {}
};
constexpr size_t kLdsNoOptIn = 64 * 1024;

// every launch of a template kernel, and every launch with dynamic LDS; the caller checks hipGetLastError
template <auto Kernel, typename... Args>
int launch_kernel(dim3 grid, dim3 block, Lds lds, hipStream_t st, Args&&... args) {  // (by reference: an owning buffer converts to its pointer at the launch itself)
    int rc;
    if (lds.bytes > kLdsNoOptIn && (rc = opt_in_lds<Kernel>(lds.opt_in)) != 0) return rc;
    hipLaunchKernelGGL(Kernel, grid, block, lds.bytes, st, args...);
    return CODD_KNN_OK;
}

// a launch of a squared-L2 kernel or of its dot-product twin (kernel_metric(): cosine and ip run Dot), where both take the same arguments.
// L2 stands first because the call sites named the l2 kernel first before this existed: the compiler emits template kernels in the
// order in which they are first named, and that order is part of the build
template <auto L2, auto Dot, typename... Args>
int launch_by_metric(int metric, dim3 grid, dim3 block, Lds lds, hipStream_t st, Args&&... args) {
    if (metric == kMetricL2) return launch_kernel<L2>(grid, block, lds, st, args...);
    return launch_kernel<Dot>(grid, block, lds, st, args...);
}

}  // namespace
