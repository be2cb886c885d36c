// engine/model_impl.h -- what the model*.cpp translation units share among themselves; not part of the engine's interface
#pragma once
#include "model.h"
#include "../../../include/ntk_engine.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace nt {

#define NT_TRY(expr)                       \
    do {                                   \
        const int st__ = (expr);           \
        if (st__ != NTK_OK) return st__;   \
    } while (0)

// The status of a pass that queues launch after launch: the FIRST failure is the pass's, the calls behind it still go out.  ok(st) folds one in.
struct PassStatus {
    int rc = NTK_OK;
    void operator()(int st) { if (st != NTK_OK && rc == NTK_OK) rc = st; }
};

inline bool is_quant(int dt) {
    return dt == NTK_DT_Q8_0 || dt == NTK_DT_Q4_0 || dt == NTK_DT_Q4_K || dt == NTK_DT_Q5_K || dt == NTK_DT_Q6_K;
}

// unquantised rows of 16-bit words: the fused decode GEMV (gemv_dense16.hip) and the F32-MFMA prompt GEMM take them beside the quantised formats
inline bool is_dense16(int dt) { return dt == NTK_DT_F16 || dt == NTK_DT_BF16; }

// the three statuses with which a launcher says "nothing was launched: try the next form"
inline bool not_taken(int st) { return st == NTK_E_DTYPE || st == NTK_E_SHAPE || st == NTK_E_ALIGN; }

// which launch kinds read the repacked tensors: 1 Q|K|V, 2 Wo, 4 gate|up, 8 down, 16 LM head (tuning builds: NTK_RP_MASK)
inline int rp_mask() {
#ifdef NTK_TUNE
    static const int m = [] { const char* e = getenv("NTK_RP_MASK"); return e ? atoi(e) : 31; }();
    return m;
#else
    return 31;
#endif
}

// device bytes behind a raw tensor of `nbytes` (tail padding: kernels may read the last 16-byte chunk whole); the unpack scratch is carved in the same units
inline size_t padded_bytes(size_t nbytes) { return (nbytes + 255) / 256 * 256 + 256; }

// What body() enqueues on `st`, captured and instantiated: *out is the executable graph.  body's own failure wins over the capture's.
template <class Body>
int capture_graph(hipStream_t st, hipStreamCaptureMode mode, Body&& body, hipGraphExec_t* out) {
    if (hipStreamBeginCapture(st, mode) != hipSuccess) return NTK_E_LAUNCH;
    int rc = body();
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &g);
    if (rc == NTK_OK && (e != hipSuccess || !g)) rc = NTK_E_LAUNCH;
    if (rc == NTK_OK && hipGraphInstantiate(out, g, nullptr, nullptr, 0) != hipSuccess) rc = NTK_E_LAUNCH;
    if (g) (void)hipGraphDestroy(g);
    return rc;
}

}  // namespace nt
