// slak_amd/pybind/block_runner.cpp -- one block of the decomposed SLaK trunk (models/SLaK.py:153-166) issued from C++: the call sequence of
// slak_amd/block_ops._BlockFn (three branch convs + BatchNorm sums -> branch BatchNorms + add -> permute + LayerNorm -> pwconv1 -> GELU ->
// pwconv2 -> gamma * + permute + residual, and its backward) as TWO host calls per block and step instead of ~70 ctypes calls, ~25 torch.empty
// and 4-6 GEMM dispatches made from Python.  Same launches on the same operands in the same order as the Python node: results are bit-identical
// (tests/test_model_reference_gpu.py::test_block_runner_issues_the_same_launches_as_the_python_node).  Host-only C++ on the C ABI of include/slak_hip.h; tensors are allocated through the torch allocator, kernels
// go to torch's CURRENT stream, the GEMMs the library does not cover are at::linear / at::mm (hipBLASLt).  Which launch runs each step of the branch convs and
// of the pointwise MLP is the library's answer (slak_tri_plan, slak_mlp_plan under the caller's `allow` masks): the Python sequence switches on the same plans.
//
// SyncBatchNorm (round 5): with an `exchange` callable (block_ops._sync_bn_all_reduce bound to the process group) the branch BatchNorms run as
// sums -> exchange -> apply: forward one blocking all-reduce of 6C+1 doubles, backward one all-reduce of 4C floats issued ASYNCHRONOUSLY in front of
// the two pointwise weight gradients and waited for behind them -- so a DDP run issues its blocks from here too, not from the Python sequence.
//
// The caches below are shared by the forward (caller thread) and the backward (autograd's device threads, possibly one per GPU in a single process):
// one mutex guards their lookups / inserts; entries are never erased, so references stay valid after the lock is dropped.
//
// Pitched blocks (odd C of the width-1.3 models, or an even width under block_ops.pad_even_widths): the NHWC intermediates t, y1, a, z and their gradients
// have rows of `ldc` > C elements, the caller hands in the zero-padded bf16 operands block_ops._pitched_operands builds (W1 [4 ldc][ldc], W2 [ldc][4 ldc], both
// transposes, b1, b2).  The convs and BatchNorms run on the logical C (any parity), the MLP on (M, 4 ldc, ldc), the tail through the slak_*_ld entry points;
// the backward cuts dW1, db1, dW2 back to the parameters' shapes.  The launches are those of the Python sequence on the same operands: bit-identical results
// (tests/test_pitched_runner_gpu.py).  ldc == C is the plain block, launch for launch what it was.
//
// block_forward returns an EMPTY list when slak_tri_plan names a rung that is not issued here (anything but the three-branch forward with statistics
// and either the one-launch backward or the three-branch data-gradient and weight-gradient launches): the caller (block_ops._BlockFn) then runs the
// Python sequence, which knows every rung.
#include <torch/extension.h>
#include <torch/csrc/distributed/c10d/ProcessGroup.hpp>
#include <torch/csrc/distributed/c10d/Types.hpp>
#include <torch/csrc/distributed/c10d/Work.hpp>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/slak_hip.h"

namespace {

using at::Tensor;

std::mutex g_cache_mu;

void* stream_of(const Tensor& t) { return (void*)c10::hip::getCurrentHIPStream(t.get_device()).stream(); }

void check_rc(int rc, const char* fn) {
    TORCH_CHECK(rc == SLAK_OK, fn, ": ", slak_status_string(rc), " (", slak_last_hip_error(), ")");
}

// The SyncBatchNorm statistics exchange: `exchange` is None (single process), a torch.distributed ProcessGroup -- the all-reduce is then issued from
// here (ProcessGroup::allreduce: ~5 us of host time, no Python frame, the GIL is not needed) -- or a Python callable(buf, async_op) -> work | None
// (block_ops._sync_bn_all_reduce behind a lambda: what the tests patch to record the order of the calls).
struct Exchange {
    pybind11::object fn;                                           // the callable form
    c10::intrusive_ptr<c10d::ProcessGroup> pg;                     // the direct form
    c10::intrusive_ptr<c10d::Work> work;                           // an asynchronous all-reduce in flight (direct form)
    pybind11::object pywork = pybind11::none();                    //                                    (callable form)
    explicit Exchange(const pybind11::object& o) {
        if (o.is_none()) return;
        if (pybind11::hasattr(o, "allreduce") && pybind11::hasattr(o, "rank")) {
            try { pg = o.cast<c10::intrusive_ptr<c10d::ProcessGroup>>(); } catch (const pybind11::cast_error&) { pg = nullptr; }
        }
        if (!pg) fn = o;
    }
    bool none() const { return !pg && !fn; }
    void run(Tensor& buf, bool async) {                            // SUM, in place
        if (pg) {
            // WITHOUT the GIL: a backend that completes work on its own threads (gloo) may have to run a Python callback there first -- DistributedDataParallel's
            // comm-hook futures -- and a host-blocking wait() under the GIL would starve it (two ranks over gloo deadlocked exactly so: round 6)
            pybind11::gil_scoped_release nogil;
            c10d::AllreduceOptions opts;
            opts.reduceOp = c10d::ReduceOp::SUM;
            opts.asyncOp = async;
            std::vector<Tensor> v{buf};
            auto w = pg->allreduce(v, opts);
            if (async) work = w; else if (w) w->wait();            // (RCCL: ordered on the current stream, no host wait; gloo: blocks the host)
        } else {
            pywork = fn(buf, async);
        }
    }
    void wait() {
        if (work) { pybind11::gil_scoped_release nogil; work->wait(); work = nullptr; }
        if (!pywork.is_none()) { pywork.attr("wait")(); pywork = pybind11::none(); }
    }
};

// per-(device, stream) scratch, grown on demand; stream-ordered reuse is safe because every kernel that touches it is enqueued on that stream
struct Scratch { void* p; size_t n; };
Scratch scratch(const Tensor& like, size_t bytes) {
    static std::map<std::pair<int, void*>, Tensor> cache;
    const auto key = std::make_pair((int)like.get_device(), stream_of(like));
    std::lock_guard<std::mutex> lk(g_cache_mu);
    auto it = cache.find(key);
    if (it == cache.end() || (size_t)it->second.numel() < bytes) {
        Tensor t = at::empty({(int64_t)std::max<size_t>(bytes, (size_t)1 << 22)}, like.options().dtype(at::kByte));
        cache[key] = t;
        return {t.data_ptr(), (size_t)t.numel()};
    }
    return {it->second.data_ptr(), (size_t)it->second.numel()};
}

// A second stream per device for work of a block's backward that nothing else in the block waits for (the two pointwise weight gradients:
// matrix-core bound at ~0.3 of their peak, little HBM traffic) beside the HBM-bound passes of the main stream.  OFF by default
// (SLAK_WGRAD_SIDE_STREAM=1 turns it on): measured 16.45-16.57 ms per SLaK-T step with it against 16.59-16.63 without in two interleaved pairs on
// one box -- inside the noise -- for 0.6-1 ms more host time per step (two event records and two stream waits per block).
struct Side { hipStream_t st = nullptr; hipEvent_t fork = nullptr, join = nullptr; bool ok = false; };
Side& side_of(int dev) {
    static std::map<int, Side> m;
    std::lock_guard<std::mutex> lk(g_cache_mu);
    auto it = m.find(dev);
    if (it != m.end()) return it->second;
    Side s;
    static const bool on = [] { const char* e = getenv("SLAK_WGRAD_SIDE_STREAM"); return e && e[0] == '1'; }();
    if (on && hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&s.fork, hipEventDisableTiming) == hipSuccess &&
        hipEventCreateWithFlags(&s.join, hipEventDisableTiming) == hipSuccess) s.ok = true;
    return m.emplace(dev, s).first->second;
}

struct Shape { int N, C, H, W, K, P, M, C4, Cp; };                  // Cp: the row pitch of the NHWC tensors (== C: a plain block); C4: rows of W1 as handed in (4 Cp)

// what the library answers for a block shape and the caller's `allow` masks (slak_mlp_plan's kernel families, slak_tri_plan's launches), asked once
struct Plan { bool ok; size_t ws; slak_tri_plan_t tri; slak_mlp_plan_t mlp; size_t off[5], len[5]; };   // off/len: the backward's deferred-reduction regions behind the common scratch
const Plan& plan_of(const Shape& s, unsigned allow, unsigned tri_allow) {
    static std::map<std::vector<int>, Plan> cache;
    const std::vector<int> key = {s.N, s.C, s.H, s.W, s.K, s.C4, s.Cp, (int)allow, (int)tri_allow};
    std::lock_guard<std::mutex> lk(g_cache_mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    Plan p{};
    // (dgrad == ONE is taken without asking slak_dwconv2d_tri_supported_op(.., 1), which the runner used to require of every block: the one-launch
    // backward exists only inside the small three-branch class, where that query says yes)
    p.ok = slak_tri_plan(SLAK_BF16, s.N, s.C, s.H, s.W, s.K, tri_allow, &p.tri) == SLAK_OK && p.tri.fwd == SLAK_TRI_FWD_TRI_STATS &&
           (p.tri.dgrad == SLAK_TRI_DGRAD_ONE || (p.tri.dgrad == SLAK_TRI_DGRAD_TRI && p.tri.wgrad == SLAK_TRI_WGRAD_TRI)) &&
           slak_mlp_plan(s.M, s.C4, s.Cp, allow, &p.mlp) == SLAK_OK;
    if (s.Cp == s.C) p.ok = p.ok && (s.C % 2) == 0 && s.C <= 1024;
    else {                                                         // pitched: any parity of C; every tail op must have a kernel for (C, ldc)
        p.ok = p.ok && s.Cp > s.C && s.Cp % 8 == 0 && s.Cp <= 1024 && s.C4 == 4 * s.Cp;
        for (int op = SLAK_TAIL_LN_FWD; op <= SLAK_TAIL_SR_BWD; ++op)
            for (int sdt : {SLAK_F32, SLAK_BF16}) p.ok = p.ok && slak_block_tail_family(op, sdt, s.N, s.C, s.P, s.Cp) != SLAK_TAIL_FAMILY_NONE;
    }
    // backward: the five calls whose final column sums are deferred into one launch keep their partial rows until then: a region each,
    // behind the scratch the other calls share -- [scale_residual][gelu'][LayerNorm][dW1][dW2]
    const auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t tail = slak_block_tail_workspace_bytes(s.N, s.Cp, s.P);
    const size_t len[5] = {tail, p.mlp.ws_dy1, tail, p.mlp.ws_dw1, p.mlp.ws_dw2};
    size_t o = up(std::max({p.tri.ws_wgrad, slak_bn3_workspace_bytes(s.N, s.C), tail, p.mlp.ws_dy1, p.mlp.ws_dw1, p.mlp.ws_dw2}));   // (the MLP launches use their regions; leaving them out here moves the regions and made the step time bimodal: profiles/mlp_plan_step_times.jsonl)
    for (int k = 0; k < 5; ++k) { p.off[k] = o; p.len[k] = up(std::max<size_t>(len[k], 256)); o += p.len[k]; }
    p.ws = o;
    return cache.emplace(key, p).first->second;
}

Shape shape_of(const Tensor& x, const Tensor& wv, const Tensor& w1b) {
    Shape s;
    s.N = (int)x.size(0); s.C = (int)x.size(1); s.H = (int)x.size(2); s.W = (int)x.size(3); s.K = (int)wv.size(2);
    s.P = s.H * s.W; s.M = s.N * s.P; s.C4 = (int)w1b.size(0); s.Cp = (int)w1b.size(1);
    return s;
}

const float* fp(const Tensor& t) { return (const float*)t.data_ptr(); }
float* fpm(const Tensor& t) { return (float*)t.data_ptr(); }

// -> [out, out16 | undefined, x16, yv, yh, ys, bnstats, s, t, mean, rstd, y1m, a, z, count_dev | undefined], or an empty list (see the header)
std::vector<Tensor> block_forward(const Tensor& x, const c10::optional<Tensor>& x_lowp, const Tensor& wv, const Tensor& wh, const Tensor& wsm,
                                  const std::vector<Tensor>& bn_gamma, const std::vector<Tensor>& bn_beta, const std::vector<Tensor>& bn_mean,
                                  const std::vector<Tensor>& bn_var, double bn_eps, double bn_momentum, bool update_running,
                                  const Tensor& lnw, const Tensor& lnb, double ln_eps, const Tensor& w1b, const Tensor& bb1b, const Tensor& w2b,
                                  const Tensor& bb2b, const Tensor& gamma, const c10::optional<Tensor>& sample_scale, bool emit_lowp,
                                  const pybind11::object& exchange_obj /* None: single process; else see Exchange */,
                                  int64_t ldc /* row pitch of the NHWC tensors; != C: w1b .. bb2b are the zero-padded operands */,
                                  int64_t allow /* SLAK_MLP_ALLOW_*: block_ops' use_skinny_linear / use_linear_gemm / use_linear_wgrad */,
                                  int64_t tri_allow /* SLAK_TRI_ALLOW_*: block_ops._tri_allow */) {
    Exchange exchange(exchange_obj);
    TORCH_CHECK(w1b.dim() == 2 && w2b.dim() == 2 && ldc == w1b.size(1) && ldc == w2b.size(0) && w2b.size(1) == w1b.size(0) && bb1b.numel() == w1b.size(0) &&
                bb2b.numel() == ldc, "the pointwise operands do not fit the pitch");
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 4, "x must be a contiguous (N,C,H,W) HIP tensor");
    TORCH_CHECK(bn_gamma.size() == 3 && bn_beta.size() == 3 && bn_mean.size() == 3 && bn_var.size() == 3, "three branch BatchNorms");
    const Shape s = shape_of(x, wv, w1b);
    const Plan& pl = plan_of(s, (unsigned)allow, (unsigned)tri_allow);
    const bool f32w = wv.scalar_type() == at::kFloat && wh.scalar_type() == at::kFloat && wsm.scalar_type() == at::kFloat && wv.is_contiguous() &&
                      wh.is_contiguous() && wsm.is_contiguous() && wv.size(3) == 5 && wh.size(2) == 5 && wh.size(3) == s.K && wsm.size(2) == 5 && wsm.size(3) == 5;
    if (!pl.ok || !f32w || (x.scalar_type() != at::kFloat && x.scalar_type() != at::kBFloat16) || w1b.scalar_type() != at::kBFloat16) return {};
    c10::hip::HIPGuard guard(x.get_device());
    void* st = stream_of(x);
    const int dt = SLAK_BF16;
    Tensor x16 = (x_lowp.has_value() && x_lowp->defined()) ? x_lowp->contiguous() : x.to(at::kBFloat16).contiguous();
    const Scratch ws = scratch(x, pl.ws);
    // three branch convs + the BatchNorms' batch sums
    Tensor yv = at::empty_like(x16), yh = at::empty_like(x16), ys = at::empty_like(x16);
    Tensor stats = at::empty({pl.tri.stats_rows, s.C, 6}, x.options().dtype(at::kFloat));
    check_rc(slak_dwconv2d_tri_forward_stats(x16.data_ptr(), fp(wv), fp(wh), fp(wsm), yv.data_ptr(), yh.data_ptr(), ys.data_ptr(), fpm(stats), dt,
                                             s.N, s.C, s.H, s.W, s.K, st), "slak_dwconv2d_tri_forward_stats");
    // branch BatchNorms + add
    const float* gam[3] = {fp(bn_gamma[0]), fp(bn_gamma[1]), fp(bn_gamma[2])};
    const float* bet[3] = {fp(bn_beta[0]), fp(bn_beta[1]), fp(bn_beta[2])};
    float* rm[3] = {fpm(bn_mean[0]), fpm(bn_mean[1]), fpm(bn_mean[2])};
    float* rv[3] = {fpm(bn_var[0]), fpm(bn_var[1]), fpm(bn_var[2])};
    const float* pre[3] = {fp(stats), fp(stats) + 2, fp(stats) + 4};
    const int pre_rows[3] = {pl.tri.stats_rows, pl.tri.stats_rows, pl.tri.stats_rows};
    Tensor coef = at::empty({s.C * 4}, stats.options()), bnstats = at::empty({s.C * 6}, stats.options());
    Tensor sum = at::empty_like(yv), count_dev;
    if (exchange.none()) {
    check_rc(slak_bn3_forward_local(yv.data_ptr(), yh.data_ptr(), ys.data_ptr(), gam, bet, rm, rv, (float)bn_eps, (float)bn_momentum, update_running ? 1 : 0,
                                    fpm(coef), fpm(bnstats), sum.data_ptr(), s.N, s.C, s.P, ws.p, ws.n, st, pre, pre_rows, 6), "slak_bn3_forward_local");
    } else {                                                       // SyncBatchNorm: the conv launches' rows feed the exchange buffer, one all-reduce, then the apply pass
        Tensor sums = at::empty({(int64_t)s.C * 6 + 1}, x.options().dtype(at::kDouble));
        check_rc(slak_bn3_forward_sums_counted(yv.data_ptr(), yh.data_ptr(), ys.data_ptr(), (double*)sums.data_ptr(), s.N, s.C, s.P, ws.p, ws.n, st, pre, pre_rows, 6),
                 "slak_bn3_forward_sums_counted");                   // (element 6C = this rank's N * P: no fill launch)
        const double count = (double)s.N * (double)s.P;
        count_dev = sums.narrow(0, (int64_t)s.C * 6, 1);           // the global element count stays on the device (no host sync)
        exchange.run(sums, false);                                 // blocking on the stream: the apply pass needs the result at once
        check_rc(slak_bn3_forward_apply(yv.data_ptr(), yh.data_ptr(), ys.data_ptr(), (const double*)sums.data_ptr(), count, (const double*)count_dev.data_ptr(),
                                        gam, bet, rm, rv, (float)bn_eps, (float)bn_momentum, 1, update_running ? 1 : 0, fpm(coef), fpm(bnstats), sum.data_ptr(),
                                        s.N, s.C, s.P, st), "slak_bn3_forward_apply");
    }
    // permute + LayerNorm (rows of Cp; Cp == C: the plain block)
    Tensor t = at::empty({s.N, s.H, s.W, s.Cp}, x16.options());
    Tensor mean = at::empty({s.N, s.P}, stats.options()), rstd = at::empty({s.N, s.P}, stats.options());
    check_rc(slak_ln_nchw_to_nhwc_forward_ld(sum.data_ptr(), fp(lnw), fp(lnb), t.data_ptr(), fpm(mean), fpm(rstd), s.N, s.C, s.P, (float)ln_eps, st, s.Cp),
             "slak_ln_nchw_to_nhwc_forward_ld");
    // pwconv1 -> GELU -> pwconv2
    Tensor y1m, a, z;
    if (pl.mlp.pw1 != SLAK_MLP_LIBRARY) { y1m = at::empty({s.N, s.H, s.W, s.C4}, x16.options()); a = at::empty_like(y1m); }
    if (pl.mlp.pw1 == SLAK_MLP_FUSED || pl.mlp.pw2 == SLAK_MLP_NT) z = at::empty({s.N, s.H, s.W, s.Cp}, x16.options());
    switch (pl.mlp.pw1) {
    case SLAK_MLP_FUSED:                                           // stage 1: pwconv1, GELU and pwconv2 in one pass
        check_rc(slak_linear_mlp_fwd(t.data_ptr(), w1b.data_ptr(), bb1b.data_ptr(), w2b.data_ptr(), bb2b.data_ptr(), y1m.data_ptr(), a.data_ptr(), z.data_ptr(),
                                     s.M, s.Cp, s.C4, st), "slak_linear_mlp_fwd");
        break;
    case SLAK_MLP_NT:
        check_rc(slak_linear_nt(t.data_ptr(), w1b.data_ptr(), bb1b.data_ptr(), y1m.data_ptr(), a.data_ptr(), s.M, s.C4, s.Cp, st), "slak_linear_nt");
        break;
    case SLAK_MLP_GEMM:                                            // stages 2-3: bias, rounding and GELU in the GEMM's epilogue
        check_rc(slak_linear_gemm(t.data_ptr(), w1b.data_ptr(), bb1b.data_ptr(), y1m.data_ptr(), a.data_ptr(), nullptr, nullptr, s.M, s.C4, s.Cp, SLAK_EPI_GELU,
                                  nullptr, 0, st), "slak_linear_gemm");
        break;
    default:
        y1m = at::linear(t, w1b, bb1b);
        a = at::gelu(y1m);
    }
    if (pl.mlp.pw1 == SLAK_MLP_FUSED) {
    } else if (pl.mlp.pw2 == SLAK_MLP_NT) {
        check_rc(slak_linear_nt(a.data_ptr(), w2b.data_ptr(), bb2b.data_ptr(), z.data_ptr(), nullptr, s.M, s.Cp, s.C4, st), "slak_linear_nt");
    } else {
        z = at::linear(a, w2b, bb2b);
        if (z.scalar_type() != at::kBFloat16) z = z.to(at::kBFloat16);
        z = z.contiguous();
    }
    // gamma * + permute + residual (+ the bf16 copy for the next block's convs)
    Tensor out = at::empty({s.N, s.C, s.H, s.W}, stats.options());
    Tensor out16 = emit_lowp ? at::empty({s.N, s.C, s.H, s.W}, x16.options()) : Tensor();
    const bool has_scale = sample_scale.has_value() && sample_scale->defined();
    check_rc(slak_scale_residual_forward_ld(x.data_ptr(), x.scalar_type() == at::kFloat ? SLAK_F32 : SLAK_BF16, z.data_ptr(), fp(gamma),
                                            has_scale ? fp(*sample_scale) : nullptr, fpm(out), emit_lowp ? out16.data_ptr() : nullptr, s.N, s.C, s.P, st, s.Cp),
             "slak_scale_residual_forward_ld");
    return {out, out16, x16, yv, yh, ys, bnstats, sum, t, mean, rstd, y1m, a, z, count_dev};
}

// A parameter gradient's destination: the caller's tensor when it gave one that the kernels can write (float32, contiguous, on the device,
// the parameter's element count, 16-byte aligned: the reduction launches store float4) -- else a fresh one.  A caller's tensor is returned as a
// NEW tensor object on the same storage (detach()): autograd's AccumulateGrad then takes it over as .grad without a copy (it deep-copies a
// gradient somebody else still holds), and DistributedDataParallel(gradient_as_bucket_view=True) finds .grad aliasing its bucket view and
// skips its per-parameter copy launch (reducer.cpp mark_variable_ready_dense).
struct GradDst {
    const std::vector<c10::optional<Tensor>>* v;
    int dev;
    bool usable(int k, int64_t numel) const {
        if (!v || (size_t)k >= v->size() || !(*v)[k].has_value() || !(*v)[k]->defined()) return false;
        const Tensor& t = *(*v)[k];
        return t.is_cuda() && t.get_device() == dev && t.scalar_type() == at::kFloat && t.is_contiguous() && t.numel() == numel &&
               ((uintptr_t)t.data_ptr() & 15) == 0;
    }
    Tensor take(int k, at::IntArrayRef shape, const at::TensorOptions& f32) const {
        int64_t n = 1; for (auto d : shape) n *= d;
        return usable(k, n) ? (*v)[k]->detach().view(shape) : at::empty(shape, f32);
    }
};

Tensor wgrad(const Tensor& dy, const Tensor& x, int M, int N1, int N2, int rung, int S, const Scratch& ws, void* st, const GradDst& gd, int slot) {
    const auto f32 = dy.options().dtype(at::kFloat);
    if (rung == SLAK_MLP_KERNEL) {
        Tensor d = gd.take(slot, {N1, N2}, f32);
        check_rc(slak_linear_wgrad(dy.data_ptr(), x.data_ptr(), fpm(d), M, N1, N2, ws.p, ws.n, st), "slak_linear_wgrad");
        return d;
    }
    // widths the row-reduction kernel does not cover (e.g. SLaK-B's 128 * 2^k): the reduction index M = N*H*W is split into S batches of a
    // library batched GEMM, the S partial products are added in fp32 -- what block_ops._mlp_wgrad does (a single GEMM with K = M runs on four
    // workgroups: measured 0.86 ms per call on stage 1); S = slak_mlp_plan's `splits`
    if (S > 1) {
        Tensor parts = at::bmm(dy.view({S, M / S, N1}).transpose(1, 2), x.view({S, M / S, N2}));
        if (gd.usable(slot, (int64_t)N1 * N2)) {                     // the fp32 sum of the splits straight into the caller's tensor (same additions)
            Tensor d = gd.take(slot, {N1, N2}, f32);
            at::sum_out(d, parts, at::IntArrayRef{0}, false, at::kFloat);
            return d;
        }
        return parts.sum(at::IntArrayRef{0}, false, at::kFloat);
    }
    return at::mm(dy.t(), x).to(at::kFloat);
}

// -> [dx, dx_lowp | undefined, dwv, dwh, dws, dg1, db1, dg2, db2, dg3, db3 (branch BatchNorms), dlnw, dlnb, dw1, db1, dw2, db2, dgamma]: the sixteen parameter
// gradients in the order of _BlockFn.forward's parameters; `grad_dst` (empty, or sixteen entries in that order, None allowed): see GradDst
std::vector<Tensor> block_backward(const Tensor& x16, const Tensor& wv, const Tensor& wh, const Tensor& wsm, const Tensor& yv, const Tensor& yh,
                                   const Tensor& ys, const std::vector<Tensor>& bn_gamma, const Tensor& bnstats, const Tensor& sum, const Tensor& lnw,
                                   const Tensor& mean, const Tensor& rstd, const Tensor& t, const Tensor& w1b, const Tensor& y1m, const Tensor& a,
                                   const Tensor& w2b, const Tensor& z, const Tensor& gamma, const c10::optional<Tensor>& sample_scale,
                                   const c10::optional<Tensor>& dout_opt, const c10::optional<Tensor>& dout16_opt, bool shortcut_bf16, bool had_lowp,
                                   const c10::optional<Tensor>& count_dev, const pybind11::object& exchange_obj, const pybind11::object& trace,
                                   const c10::optional<Tensor>& w1t_opt, const c10::optional<Tensor>& w2t_opt /* cached transposed bf16 weights, or None */,
                                   const c10::optional<Tensor>& w1p_opt /* W1^T in fragment-major order (slak_linear_nt_gelu_bwd_dt), or None */,
                                   const std::vector<c10::optional<Tensor>>& grad_dst, int64_t ldc, int64_t allow, int64_t tri_allow /* as in block_forward */,
                                   bool bn_bwd_async /* block_ops._bn_bwd_async: the backward statistics exchange on the collective's own stream */) {
    Exchange exchange(exchange_obj);
    const Shape s = shape_of(x16, wv, w1b);
    TORCH_CHECK(ldc == s.Cp && z.size(-1) == ldc && t.size(-1) == ldc, "the saved tensors do not fit the pitch");
    const bool pitched = s.Cp != s.C;
    TORCH_CHECK(grad_dst.empty() || grad_dst.size() == 16, "grad_dst: empty, or one entry (tensor or None) per parameter of the block");
    const GradDst gd{grad_dst.empty() ? nullptr : &grad_dst, (int)x16.get_device()};
    const GradDst gdm = pitched ? GradDst{nullptr, (int)x16.get_device()} : gd;       // dW1, db1, dW2 of a pitched block come out padded and are cut at the end
    enum { G_WV, G_WH, G_WS, G_G1, G_B1, G_G2, G_B2, G_G3, G_B3, G_LNW, G_LNB, G_W1, G_BB1, G_W2, G_BB2, G_GAMMA };
    const Plan& pl = plan_of(s, (unsigned)allow, (unsigned)tri_allow);
    TORCH_CHECK(pl.ok, "block_backward: slak_tri_plan names a rung that is not issued here (block_forward would have declined the block)");
    c10::hip::HIPGuard guard(x16.get_device());
    void* st = stream_of(x16);
    const int dt = SLAK_BF16;
    const Scratch ws = scratch(x16, pl.ws);
    const auto region = [&](int k) { return Scratch{(char*)ws.p + pl.off[k], pl.len[k]}; };
    const auto f32 = x16.options().dtype(at::kFloat);
    // the parameter gradients' final column sums (five small launches, each alone on the GPU) are recorded and run as ONE launch at the end
    struct Deferred { bool on; Deferred() : on(slak_defer_reductions_begin() == SLAK_OK) {} int end() { const bool o = on; on = false; return o ? slak_defer_reductions_end() : SLAK_OK; }
                      ~Deferred() { if (on) (void)slak_defer_reductions_end(); } } deferred;
    // gamma * + permute + residual
    Tensor dout = (dout_opt.has_value() && dout_opt->defined()) ? dout_opt->contiguous() : at::zeros({s.N, s.C, s.H, s.W}, f32);
    if (dout.scalar_type() != at::kFloat) dout = dout.to(at::kFloat);
    Tensor dout16 = (dout16_opt.has_value() && dout16_opt->defined()) ? dout16_opt->contiguous() : Tensor();
    if (dout16.defined() && dout16.scalar_type() != at::kBFloat16) dout16 = dout16.to(at::kBFloat16);
    Tensor dsum = dout16.defined() ? at::empty_like(dout) : Tensor();
    Tensor dz = at::empty_like(z), dgamma = gd.take(G_GAMMA, {s.C}, f32), dzc = gd.take(G_BB2, {s.C}, f32);
    const bool has_scale = sample_scale.has_value() && sample_scale->defined();
    // (a pitched block's final reduction that the library cannot defer runs at once: the same sums)
    check_rc(slak_scale_residual_backward_ld(fp(dout), dout16.defined() ? dout16.data_ptr() : nullptr, dsum.defined() ? fpm(dsum) : nullptr, z.data_ptr(),
                                             fp(gamma), has_scale ? fp(*sample_scale) : nullptr, dz.data_ptr(), fpm(dgamma), fpm(dzc), s.N, s.C, s.P,
                                             region(0).p, region(0).n, st, s.Cp), "slak_scale_residual_backward_ld");
    Tensor dshortcut = dsum.defined() ? dsum : dout;
    if (shortcut_bf16) dshortcut = dshortcut.to(at::kBFloat16);
    // the MLP's data path: dz -> dact -> (GELU') dy1 (+ pwconv1's bias gradient) -> dt
    Tensor dz2 = dz.view({s.M, s.Cp});
    const auto w2t_of = [&] { return (w2t_opt.has_value() && w2t_opt->defined()) ? *w2t_opt : w2b.t().contiguous(); };
    const auto w1t_of = [&] { return (w1t_opt.has_value() && w1t_opt->defined()) ? *w1t_opt : w1b.t().contiguous(); };
    Tensor dact, dy1, dt_, db1 = gdm.take(G_BB1, {s.C4}, f32);
    const Tensor w2t = pl.mlp.dy1 != SLAK_MLP_LIBRARY ? w2t_of() : Tensor();
    if (pl.mlp.dy1 == SLAK_MLP_NT) dact = at::empty({s.M, s.C4}, x16.options()); else if (pl.mlp.dy1 != SLAK_MLP_LIBRARY) dy1 = at::empty({s.M, s.C4}, x16.options());
    switch (pl.mlp.dy1) {
    case SLAK_MLP_FUSED_DT:                                        // stage 1: FUSED with dt = dy1 W1 taken from the dy1 tiles while they are on chip
        TORCH_CHECK(w1p_opt.has_value() && w1p_opt->defined(), "block_backward: slak_mlp_plan chose slak_linear_nt_gelu_bwd_dt, the caller gave no packed W1^T");
        dt_ = at::empty({s.M, s.Cp}, x16.options());
        check_rc(slak_linear_nt_gelu_bwd_dt(dz2.data_ptr(), w2t.data_ptr(), y1m.data_ptr(), w1p_opt->data_ptr(), dy1.data_ptr(), dt_.data_ptr(), fpm(db1), s.M, s.C4,
                                            s.Cp, region(1).p, region(1).n, st), "slak_linear_nt_gelu_bwd_dt");
        break;
    case SLAK_MLP_FUSED:                                           // stage 1: dz W2, GELU' and pwconv1's bias gradient in one pass
        check_rc(slak_linear_nt_gelu_bwd(dz2.data_ptr(), w2t.data_ptr(), y1m.data_ptr(), dy1.data_ptr(), fpm(db1), s.M, s.C4, s.Cp, region(1).p, region(1).n, st),
                 "slak_linear_nt_gelu_bwd");
        break;
    case SLAK_MLP_GEMM:                                            // stages 2-3: dz W2 with GELU' and pwconv1's bias gradient in the GEMM's epilogue
        check_rc(slak_linear_gemm(dz2.data_ptr(), w2t.data_ptr(), nullptr, dy1.data_ptr(), nullptr, y1m.data_ptr(), fpm(db1), s.M, s.C4, s.Cp, SLAK_EPI_DGELU,
                                  region(1).p, region(1).n, st), "slak_linear_gemm");
        break;
    case SLAK_MLP_NT:
        check_rc(slak_linear_nt(dz2.data_ptr(), w2t.data_ptr(), nullptr, dact.data_ptr(), nullptr, s.M, s.C4, s.Cp, st), "slak_linear_nt");
        break;
    default:
        dact = at::mm(dz2, w2b);
    }
    if (dact.defined()) {                                          // the NT and LIBRARY rungs: GELU' and pwconv1's bias gradient as a pass of their own
        dy1 = at::empty_like(dact);
        check_rc(slak_gelu_backward_bias(dact.data_ptr(), y1m.data_ptr(), dy1.data_ptr(), fpm(db1), s.M, s.C4, region(1).p, region(1).n, st), "slak_gelu_backward_bias");
    }
    if (pl.mlp.dy1 == SLAK_MLP_FUSED_DT) {
    } else if (pl.mlp.dt == SLAK_MLP_NT) {
        Tensor w1t = w1t_of();
        dt_ = at::empty({s.M, s.Cp}, x16.options());
        check_rc(slak_linear_nt(dy1.data_ptr(), w1t.data_ptr(), nullptr, dt_.data_ptr(), nullptr, s.M, s.Cp, s.C4, st), "slak_linear_nt");
    } else dt_ = at::mm(dy1, w1b);
    // permute + LayerNorm
    Tensor ds = at::empty_like(sum), dlnw = gd.take(G_LNW, {s.C}, f32), dlnb = gd.take(G_LNB, {s.C}, f32);
    check_rc(slak_ln_nchw_to_nhwc_backward_ld(dt_.data_ptr(), sum.data_ptr(), fp(lnw), fp(mean), fp(rstd), ds.data_ptr(), fpm(dlnw), fpm(dlnb), s.N, s.C, s.P,
                                              region(2).p, region(2).n, st, s.Cp), "slak_ln_nchw_to_nhwc_backward_ld");
    // SyncBatchNorm: the backward sums and their all-reduce go out FIRST (asynchronously); the weight gradients below do not depend on them
    const float* gam[3] = {fp(bn_gamma[0]), fp(bn_gamma[1]), fp(bn_gamma[2])};
    Tensor bcoef = at::empty({s.C * 9}, f32);
    Tensor dgb[6];                                                 // dg1, db1, dg2, db2, dg3, db3: the caller's tensors, or rows of one [6][C] allocation
    {
        Tensor rows;
        for (int k = 0; k < 6; ++k) {
            if (gd.usable(G_G1 + k, s.C)) { dgb[k] = gd.take(G_G1 + k, {s.C}, f32); continue; }
            if (!rows.defined()) rows = at::empty({6, s.C}, f32);
            dgb[k] = rows.select(0, k);
        }
    }
    float* const dgam3[3] = {fpm(dgb[0]), fpm(dgb[2]), fpm(dgb[4])};
    float* const dbet3[3] = {fpm(dgb[1]), fpm(dgb[3]), fpm(dgb[5])};
    Tensor d1 = at::empty_like(yv), d2 = at::empty_like(yv), d3 = at::empty_like(yv);
    Tensor lsums, gsums;
    if (!exchange.none()) {
        lsums = at::empty({(int64_t)s.C * 4}, f32);
        gsums = at::empty({(int64_t)s.C * 4}, f32);                 // the all-reduce's buffer: written by the same launch (no clone)
        check_rc(slak_bn3_backward_sums_dup(ds.data_ptr(), yv.data_ptr(), yh.data_ptr(), ys.data_ptr(), fp(bnstats), fpm(lsums), fpm(gsums), s.N, s.C, s.P, ws.p, ws.n, st),
                 "slak_bn3_backward_sums_dup");
        // on the compute stream like the forward exchange (no stream hand-offs; the collective's latency is on the stream; the default since round 6), or
        // bn_bwd_async: asynchronously (its own stream: the two weight-gradient launches below run beside it)
        exchange.run(gsums, bn_bwd_async);
    }
    // the two pointwise weight gradients (single process: in front of the BatchNorm pass, as the Python node launches them)
    // (with both on the library's kernel: on the side stream, joined at the end of this function -- their operands are complete on the main
    // stream at the fork, their outputs, operands and workspace regions are not touched by the main stream before the join)
    if (!trace.is_none()) trace("pointwise_wgrads");
    Side& sd = side_of(x16.get_device());
    const bool forked = sd.ok && pl.mlp.dw1 == SLAK_MLP_KERNEL && pl.mlp.dw2 == SLAK_MLP_KERNEL && hipEventRecord(sd.fork, (hipStream_t)st) == hipSuccess && hipStreamWaitEvent(sd.st, sd.fork, 0) == hipSuccess;
    void* wst = forked ? (void*)sd.st : st;
    Tensor dw1 = wgrad(dy1, t.view({s.M, s.Cp}), s.M, s.C4, s.Cp, pl.mlp.dw1, pl.mlp.splits, region(3), wst, gdm, G_W1);
    Tensor dw2 = wgrad(dz2, a.view({s.M, s.C4}), s.M, s.Cp, s.C4, pl.mlp.dw2, pl.mlp.splits, region(4), wst, gdm, G_W2);
    struct Join { Side* sd; void* st; bool on;
                  void now() { if (on && hipEventRecord(sd->join, sd->st) == hipSuccess) (void)hipStreamWaitEvent((hipStream_t)st, sd->join, 0); on = false; }
                  ~Join() { now(); } } join{&sd, st, forked};
    check_rc(deferred.end(), "slak_defer_reductions_end");         // one launch: dgamma, db2 | db1 | dlnw, dlnb | dW1 | dW2
    if (pitched) {
        // dW1, db1, dW2 cut back to the parameters' shapes as contiguous fp32 (the pad rows and columns hold zeros) -- into the caller's tensor where one is
        // usable.  Behind the deferred reductions, which finish them, and behind the side stream's join.
        join.now();
        const auto cut = [&](const Tensor& full, int slot, int64_t r, int64_t c) {
            Tensor src = c > 0 ? full.narrow(0, 0, r).narrow(1, 0, c) : full.narrow(0, 0, r);
            if (!gd.usable(slot, c > 0 ? r * c : r)) return src.contiguous();
            Tensor d = c > 0 ? gd.take(slot, {r, c}, f32) : gd.take(slot, {r}, f32);
            d.copy_(src);
            return d;
        };
        dw1 = cut(dw1, G_W1, 4 * (int64_t)s.C, s.C);
        db1 = cut(db1, G_BB1, 4 * (int64_t)s.C, 0);
        dw2 = cut(dw2, G_W2, s.C, 4 * (int64_t)s.C);
    }
    // branch BatchNorms
    if (exchange.none()) {
    check_rc(slak_bn3_backward_local_to(ds.data_ptr(), yv.data_ptr(), yh.data_ptr(), ys.data_ptr(), fp(bnstats), gam, fpm(bcoef), dgam3, dbet3,
                                        d1.data_ptr(), d2.data_ptr(), d3.data_ptr(), s.N, s.C, s.P, ws.p, ws.n, st), "slak_bn3_backward_local_to");
    } else {
        exchange.wait();                                           // (asynchronous form) stream-side wait (RCCL) / host wait (gloo): the weight gradients are already queued
        const bool has_cd = count_dev.has_value() && count_dev->defined();
        check_rc(slak_bn3_backward_apply_to(ds.data_ptr(), yv.data_ptr(), yh.data_ptr(), ys.data_ptr(), fp(gsums), fp(lsums), (double)s.N * (double)s.P,
                                            has_cd ? (const double*)count_dev->data_ptr() : nullptr, fp(bnstats), gam, fpm(bcoef), dgam3, dbet3,
                                            d1.data_ptr(), d2.data_ptr(), d3.data_ptr(), s.N, s.C, s.P, st), "slak_bn3_backward_apply_to");
    }
    // three branch convs: the summed data gradient, the three weight gradients
    Tensor dx16 = at::empty_like(x16);
    Tensor dwv = gd.take(G_WV, wv.sizes(), f32), dwh = gd.take(G_WH, wh.sizes(), f32), dws = gd.take(G_WS, wsm.sizes(), f32);
    if (pl.tri.dgrad == SLAK_TRI_DGRAD_ONE) {                      // 14 x 14 class: data gradient and the three weight gradients in one launch
        check_rc(slak_dwconv2d_tri_backward(d1.data_ptr(), d2.data_ptr(), d3.data_ptr(), x16.data_ptr(), fp(wv), fp(wh), fp(wsm), dx16.data_ptr(),
                                            fpm(dwv), fpm(dwh), fpm(dws), dt, s.N, s.C, s.H, s.W, s.K, ws.p, ws.n, st), "slak_dwconv2d_tri_backward");
    } else {
    check_rc(slak_dwconv2d_tri_backward_data(d1.data_ptr(), d2.data_ptr(), d3.data_ptr(), fp(wv), fp(wh), fp(wsm), dx16.data_ptr(), dt,
                                             s.N, s.C, s.H, s.W, s.K, st), "slak_dwconv2d_tri_backward_data");
    check_rc(slak_dwconv2d_tri_backward_filter(d1.data_ptr(), d2.data_ptr(), d3.data_ptr(), x16.data_ptr(), fpm(dwv), fpm(dwh), fpm(dws), dt,
                                               s.N, s.C, s.H, s.W, s.K, ws.p, ws.n, st), "slak_dwconv2d_tri_backward_filter");
    }
    Tensor dx = had_lowp ? dshortcut : (dshortcut + dx16);
    return {dx, had_lowp ? dx16 : Tensor(), dwv, dwh, dws, dgb[0], dgb[1], dgb[2], dgb[3], dgb[4], dgb[5], dlnw, dlnb, dw1, db1, dw2, dzc, dgamma};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    // compiled against one argument list per entry point: a library built from another header must not be called through it
    if (slak_version() != SLAK_ABI_VERSION)
        throw pybind11::import_error("_slak_block_runner_C was compiled against SLAK_ABI_VERSION " + std::to_string(SLAK_ABI_VERSION) + ", libslak_hip.so reports " +
                                     std::to_string(slak_version()) + ": rebuild with `python -m slak_amd.build --pybind`");
    m.attr("abi_version") = SLAK_ABI_VERSION;
    m.def("block_forward", &block_forward, "one SLaK block, training forward (see slak_amd/block_ops._BlockFn)");
    m.def("block_backward", &block_backward, "its backward");
    // tests: the statistics exchange alone (any device the group's backend takes) -> true when the ProcessGroup was called from C++
    m.def("_exchange_probe", [](const pybind11::object& exchange, Tensor buf, bool async) {
        Exchange e(exchange);
        if (e.none()) return false;
        e.run(buf, async);
        e.wait();
        return (bool)e.pg;
    });
}
