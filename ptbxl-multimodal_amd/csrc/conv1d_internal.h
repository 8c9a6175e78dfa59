// conv1d_internal.h — what the translation units of the convolution family (conv1d_api.hip, conv1d_direct.hip,
// conv1d_mfma.hip, conv1d_mfma_bf16.hip, conv1d_bf16_ring.hip, conv1d_bf16_eval.hip, conv1d_wgrad_bf16_tk.hip) share on
// the host: every function that crosses a file, grouped by the file that defines it, and the types that travel with
// them.  The defining file includes this header too, so a definition that drifts from its declaration does not compile.
// A host function that is not here is `static` (or in an anonymous namespace) in its file:
// tests/test_csrc_interfaces_host.py refuses a prototype written into a source file and a type defined twice.
#pragma once
#include "common.h"
#include "wgrad_reduce.h"

namespace ecg {

// conv1d_direct.hip
int direct_fwd_stat_partials(int N, int Lo);
int direct_fwd(const float *x, const float *wp, const float *bias, float *y, float *partials,
               int N, int Cin, int Cout, int L, int K, int pad, hipStream_t st);
int direct_wgrad_splits(int N, int Cin, int Cout, int K);
size_t direct_wgrad_ws_floats(int N, int Cin, int Cout, int K);
int direct_wgrad(const float *dy, const float *x, float *dw, float *db, float *ws, int N, int Cin,
                 int Cout, int L, int K, int pad, hipStream_t st);
int direct_wgrad_slabs(const float *dy, const float *x, float *dw, float *db, float *ws, int N, int Cin,
                       int Cout, int L, int K, int pad, hipStream_t st, WgradReduce *red);
int pack_weights(const float *w, float *w_fwd, float *w_bwd, int Co, int Ci, int K,
                 hipStream_t st);
int pack_weights_grouped(const float *const *w, float *const *w_fwd, float *const *w_bwd, void *const *wb_fwd,
                         void *const *wb_bwd, const int *Co, const int *Ci, const int *K, int count, hipStream_t st);
// dw[i] = sum_s slab[s][i] in fixed order: which form sums a slab set, its standalone launch, and both in one call
WgradReduce wgrad_reduce_describe(const float *ws, float *dw, float *db, size_t wslab, int Cin, int Cout, int S);
int wgrad_reduce_launch(const WgradReduce &r, hipStream_t st);
int wgrad_reduce(const float *ws, float *dw, float *db, size_t wslab, int Cout, int S, hipStream_t st);

// conv1d_mfma.hip
bool mfma_fwd_supported(int Cin, int Cout, int K, int pad);
int mfma_fwd_stat_partials(int N, int Cin, int Cout, int Lo);
int mfma_fwd(const float *x, int ldx, const float *wp, const float *bias, float *y, float *partials,
             int N, int Cin, int Cout, int L, int K, int pad, hipStream_t st);
int mfma_fwd_rider(const float *x, int ldx, const float *wp, float *y, int N, int Cin, int Cout, int L, int K, int pad,
                   WgradReduce red, hipStream_t st);
int mfma_fwd_eval_pool(const float *x, const float *wp, const float *bias, const float *gamma,
                       const float *beta, const float *mean, const float *var, float eps, float *p,
                       int N, int Cin, int Cout, int L, int K, int pad, hipStream_t st, int gap);
bool mfma_fwd_eval_gap_supported(int Cin, int Cout, int L, int K, int pad);
bool mfma_wgrad_supported(int Cin, int Cout, int K);
size_t mfma_wgrad_ws_floats(int N, int Cin, int Cout, int L, int K, int pad);
int mfma_wgrad_dma_stride(int Lo, int tt);
int mfma_multiplies_per_pair(int op, int Cin, int Cout, int K, int pad);
int mfma_wgrad(const float *dy, int ldy, const float *x, float *dw, float *db, float *ws, int N,
               int Cin, int Cout, int L, int K, int pad, hipStream_t st);
int mfma_wgrad_slabs(const float *dy, int ldy, const float *x, float *dw, float *db, float *ws, int N,
                     int Cin, int Cout, int L, int K, int pad, hipStream_t st, WgradReduce *red);
int mfma_wgrad_reduce(const WgradReduce &red, hipStream_t st);
void mfma_wgrad_form(const float *dy, int ldy, int N, int Cin, int Cout, int L, int K, int pad, int form[4], size_t *slab_floats);

// conv1d_bf16_ring.hip
// What a launch of the ring kernel is planned as: the tile (co_t x t_t), the chunks of the weight slice kept resident
// (0: the ring), the persistent workgroups per C_out tile, and whether x is the fp32 network input.
struct RingPlan { bool ok; int co_t, t_t, res_ch, G; bool xf32; };
namespace ring {
// EPI: what the kernel's epilogue writes (conv1d_bf16_ring_kernel); the eval forms report the value (ecg_hip.h)
enum Epilogue { EPI_Y = 0, EPI_PH = 1, EPI_PF = 2, EPI_GAP = 3 };
}  // namespace ring
RingPlan bf16_ring_plan(int N, int Cin, int Cout, int Lo, int K, int pad, int ldx, int ldyo, bool xf32 = false);
int bf16_ring_launch(const RingPlan &p, const void *x, int ldx, const void *wb, const float *bias, void *y, int ldyo,
                     float *partials, int P_stride, int N, int Cin, int Cout, int L, int Lo, int pad, hipStream_t st);
int bf16_eval_launch(const RingPlan &p, ring::Epilogue epi, const void *x, int ldx, const void *wb,
                     const float *gamma, const float *beta, const float *mean, const float *var, float eps,
                     const float *bias, void *p_bf16, int ldp, float *out, int N, int Cin, int Cout, int L, int Lo, int pad,
                     hipStream_t st);

// conv1d_wgrad_bf16_tk.hip
bool wgrad_bf16_tk_supported(int Cin, int Cout, int K, int pad);

// Persistent grids (bf16_cfg, bf16_ring_plan, bf16_eval_plan): of `slots` resident workgroups per C_out tile, the FEWEST
// whose busiest member still has no more of the ntiles (n, t-tile) tiles than the busiest of `slots` would
inline int persistent_groups(long long slots, long long ntiles) {
    long long G = slots < ntiles ? slots : ntiles;
    if (G < 1) G = 1;
    const long long per = (ntiles + G - 1) / G;       // tiles of the busiest workgroup
    return (int)((ntiles + per - 1) / per);           // fewest workgroups with that maximum
}

}  // namespace ecg
