// slak_amd/csrc/tri_plan.hip -- slak_tri_plan: which entry point runs each step of a block's three branch convs (models/SLaK.py:82-100).  Host code only.
// The ladder of include/slak_hip.h written once, from the public slak_dwconv2d_tri_* / _pair_* queries of capi.hip (which keeps deciding which kernel
// exists); slak_amd/block_ops.py and slak_amd/pybind/block_runner.cpp switch on the answer.  A new launch for one of the steps is a new rung HERE and a
// new case in the two callers' switches -- no caller assembles a policy of its own.
#include "slak_common.h"

extern "C" int slak_tri_plan(int dtype, int N, int C, int H, int W, int K, unsigned allow, slak_tri_plan_t* plan) {
    if (!plan || N <= 0 || C <= 0 || H <= 0 || W <= 0 || K <= 0) return SLAK_ERR_INVALID_ARG;
    const bool fused = allow & SLAK_TRI_ALLOW_FUSED, stats = allow & SLAK_TRI_ALLOW_STATS, wgrad = allow & SLAK_TRI_ALLOW_WGRAD;
    const size_t tri_bytes = slak_dwconv2d_tri_filter_workspace_bytes(dtype, N, C, H, W, K);
    const size_t pair_bytes = slak_dwconv2d_pair_filter_workspace_bytes(dtype, N, C, H, W, K);
    const int rows = slak_dwconv2d_tri_stats_rows(dtype, N, C, H, W, K);
    const bool one = fused && wgrad && (allow & SLAK_TRI_ALLOW_BACKWARD) && tri_bytes > 0 && slak_dwconv2d_tri_backward_supported(dtype, N, C, H, W, K) == 1;
    slak_tri_plan_t p = {};
    p.fwd = fused && slak_dwconv2d_tri_supported_op(dtype, N, C, H, W, K, 0) == 1 ? (stats && rows > 0 ? SLAK_TRI_FWD_TRI_STATS : SLAK_TRI_FWD_TRI)
          : stats                                                                 ? SLAK_TRI_FWD_BRANCH_STATS : SLAK_TRI_FWD_BRANCH;
    p.stats_rows = p.fwd == SLAK_TRI_FWD_TRI_STATS ? rows : 0;
    p.dgrad = one                                                                 ? SLAK_TRI_DGRAD_ONE
            : fused && slak_dwconv2d_tri_supported_op(dtype, N, C, H, W, K, 1) == 1 ? SLAK_TRI_DGRAD_TRI
            : (allow & SLAK_TRI_ALLOW_DGRAD_ACC)                                  ? SLAK_TRI_DGRAD_BRANCH_ACC : SLAK_TRI_DGRAD_BRANCH_ADD;
    p.wgrad = one                     ? SLAK_TRI_WGRAD_ONE
            : wgrad && tri_bytes > 0  ? SLAK_TRI_WGRAD_TRI
            : wgrad && pair_bytes > 0 ? SLAK_TRI_WGRAD_PAIR : SLAK_TRI_WGRAD_BRANCH;
    p.ws_wgrad = (p.wgrad == SLAK_TRI_WGRAD_ONE || p.wgrad == SLAK_TRI_WGRAD_TRI) ? tri_bytes : p.wgrad == SLAK_TRI_WGRAD_PAIR ? pair_bytes : 0;
    *plan = p;
    return SLAK_OK;
}
