// Internal glue: the public ABI (include/tavhip.h), the host decisions (entry_plan.h) and the launch helpers every enqueue uses.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"
#include "entry_plan.h"

#define TAV_ABI_VERSION 7

static inline int tav_last_error() { return (int)hipGetLastError(); }

// One launch with the geometry of a plan::Launch, and its status looked at right away: an entry of several kernels stops at the first
// that could not be enqueued.  The enclosing function (or dispatch lambda) returns int; it ends with `return 0`.
#define TAV_LAUNCH(kernel, L, stream, ...)                                                                                              \
    do {                                                                                                                                \
        hipLaunchKernelGGL(kernel, dim3((unsigned)(L).gx, (unsigned)(L).gy, (unsigned)(L).gz), dim3((L).block), (L).lds, (hipStream_t)(stream), __VA_ARGS__); \
        if (const int tav_e_ = tav_last_error()) return tav_e_;                                                                         \
    } while (0)

namespace tav {
// ABI dtype code -> element type
template <int CODE> struct elem;
template <> struct elem<TAV_F32> { using type = float; };
template <> struct elem<TAV_BF16> { using type = bf16; };
template <> struct elem<TAV_U8> { using type = uint8_t; };
template <> struct elem<TAV_I16> { using type = int16_t; };
// One accepted case of an entry: a dtype code, or a (source, destination) pair of them.
template <int A, int B = -1> struct on {
    static bool match(int a, int b) { return a == A && (B < 0 || b == B); }
    template <typename F> static int call(F& f) {
        if constexpr (B < 0) return f(typename elem<A>::type());
        else return f(typename elem<A>::type(), typename elem<(B < 0 ? A : B)>::type());
    }
};
// THE dtype dispatch: dtypes<cases...>::dispatch(code, f) or (source code, destination code, f) calls the generic callable f with a value
// of the element type(s) of the first case that matches and returns what it returns; TAV_ERR_DTYPE for codes the entry does not list.
// The kernels a callable names are instantiated in the order of the cases.
template <typename... Cases> struct dtypes {
    template <typename F> static int dispatch(int a, int b, F&& f) {
        int rc = TAV_ERR_DTYPE;
        (void)(... || (Cases::match(a, b) && ((rc = Cases::call(f)), true)));       // (a left fold: the cases are instantiated first to last)
        return rc;
    }
    template <typename F> static int dispatch(int a, F&& f) { return dispatch(a, -1, f); }
};
using floats = dtypes<on<TAV_BF16>, on<TAV_F32>>;      // what most entries take, in the order their kernels lie in the code object
}  // namespace tav
