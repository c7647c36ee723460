// slak_amd/csrc/mlp_plan.hip -- slak_mlp_plan: which launch runs each step of a block's pointwise MLP (models/SLaK.py:158-160).  Host code only.
// The ladder of include/slak_hip.h written once, from the support and size queries of linear_skinny.hip, linear_gemm.hip, linear_wgrad.hip and
// block_tail.hip (the launches validate with the same queries); slak_amd/block_ops.py and slak_amd/pybind/block_runner.cpp switch on the answer.
// A new kernel for one of the steps is a new rung HERE and a new case in the two callers' switches -- no caller assembles a policy of its own.
#include "slak_common.h"

using namespace slak;

extern "C" int slak_mlp_plan(int M, int C4, int Cp, unsigned allow, slak_mlp_plan_t* plan) {
    if (!plan || M <= 0 || C4 <= 0 || Cp <= 0) return SLAK_ERR_INVALID_ARG;
    static const int rows = [] { const char* e = getenv("SLAK_SPLITK_ROWS"); return e ? atoi(e) : 6272; }();   // rows per split of a LIBRARY weight gradient
    const bool skinny = allow & SLAK_MLP_ALLOW_SKINNY, gemm = allow & SLAK_MLP_ALLOW_GEMM, wgrad = allow & SLAK_MLP_ALLOW_WGRAD;
    slak_mlp_plan_t p = {};
    p.pw1 = skinny && slak_linear_mlp_fwd_supported(M, Cp, C4)            ? SLAK_MLP_FUSED
          : skinny && slak_linear_nt_supported(M, C4, Cp, 1)              ? SLAK_MLP_NT
          : gemm && slak_linear_gemm_supported(M, C4, Cp, SLAK_EPI_GELU)  ? SLAK_MLP_GEMM : SLAK_MLP_LIBRARY;
    p.pw2 = skinny && slak_linear_nt_supported(M, Cp, C4, 0)              ? SLAK_MLP_NT : SLAK_MLP_LIBRARY;
    p.dy1 = skinny && slak_linear_nt_gelu_bwd_dt_supported(M, C4, Cp)     ? SLAK_MLP_FUSED_DT      // (implies slak_linear_nt_gelu_bwd_supported)
          : skinny && slak_linear_nt_gelu_bwd_supported(M, C4, Cp)        ? SLAK_MLP_FUSED
          : gemm && slak_linear_gemm_supported(M, C4, Cp, SLAK_EPI_DGELU) ? SLAK_MLP_GEMM
          : skinny && slak_linear_nt_supported(M, C4, Cp, 0)              ? SLAK_MLP_NT : SLAK_MLP_LIBRARY;
    p.dt  = skinny && slak_linear_nt_supported(M, Cp, C4, 0)              ? SLAK_MLP_NT : SLAK_MLP_LIBRARY;
    p.dw1 = wgrad && slak_linear_wgrad_supported(M, C4, Cp)               ? SLAK_MLP_KERNEL : SLAK_MLP_LIBRARY;
    p.dw2 = wgrad && slak_linear_wgrad_supported(M, Cp, C4)               ? SLAK_MLP_KERNEL : SLAK_MLP_LIBRARY;
    p.splits = rows > 0 ? (M / rows > 1 ? M / rows : 1) : 1;
    while (p.splits > 1 && M % p.splits) --p.splits;
    p.ws_dy1 = (p.dy1 == SLAK_MLP_FUSED_DT || p.dy1 == SLAK_MLP_FUSED) ? slak_linear_nt_gelu_bwd_workspace_bytes(M, C4, Cp)
             : p.dy1 == SLAK_MLP_GEMM ? slak_linear_gemm_workspace_bytes(M, C4, Cp, SLAK_EPI_DGELU) : slak_gelu_bwd_workspace_bytes(M, C4);
    p.ws_dw1 = p.dw1 == SLAK_MLP_KERNEL ? slak_linear_wgrad_workspace_bytes(M, C4, Cp) : 0;
    p.ws_dw2 = p.dw2 == SLAK_MLP_KERNEL ? slak_linear_wgrad_workspace_bytes(M, Cp, C4) : 0;
    *plan = p;
    return SLAK_OK;
}
