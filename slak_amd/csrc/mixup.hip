// slak_amd/csrc/mixup.hip -- Mixup / CutMix of a batch on the device (main.py:296-299 builds timm's Mixup, engine.py:49-50 applies it to every batch):
// the image pass of timm1/data/mixup.py:159-207 (_mix_elem / _mix_pair / _mix_batch) and the soft targets of timm1/data/mixup.py:17-27
// (one_hot / mixup_target), one launch each (include/slak_hip.h).  The random numbers stay on the host (slak_amd/mixup.py): a launch gets
// finished per-image records -- kind, the two fp32 coefficients, the box -- by value when the whole batch shares one, else as a device table.
//
// Images.  Image n is paired with j = N-1-n and BOTH are rewritten in place from BOTH originals (in 'elem' mode with different coefficients and
// different boxes), so one workgroup row (blockIdx.y) owns a pair and one thread owns the same offsets of its two images: it loads both values, then
// stores both.  No clone, no second pass.  mixup is round(x a) + round(x_j b) -- torch's two multiplies and an add, never an fma (__fmul_rn /
// __fadd_rn, and the library is built with -ffp-contract=off).  cutmix COPIES the partner's bits inside the box and touches nothing outside it
// (1 x + 0 x_j would turn a partner's inf / NaN into NaN here and -0.0 into +0.0); a pair without a mixup record visits only the rows and columns
// its boxes cover.  An image of C H W floats need not start on 16 bytes (3 x 7 x 9 = 189) and a box row starts at any xl: the work is cut into the
// 16-byte pieces of image n's address grid, whole pieces move as float4 (image j too when it shares the alignment, else as four floats), the pieces
// a row's ends cut through move float by float.
//
// Targets.  out[n][k] = v(y_n, k) a_n + v(y_j, k) b_n, v = on where k == y, else off, over the flat (N, K) array in 16-byte pieces.  A label never
// forms an address: it is compared with the column index, so a label outside [0, K) matches no column and its row gets off-values only (torch's
// scatter_ asserts on the device there).
#include "slak_common.h"

namespace slak {

constexpr int MX_T = 256;
constexpr int MX_PIECES = 4;                                    // 16-byte pieces a thread is sized for (grid-stride loop)
constexpr long long MX_MAX_IMAGE = 1ll << 28;                   // C H W floats of one image: offsets and piece counts stay in int
constexpr int MX_MAX_N = 2 * 65535;                             // one grid row per pair

typedef slak_mixup_record_t mx_rec;

// what the kernel acts on: an unknown kind or an empty box is 'untouched', a box is clipped to the image (a table comes from device memory unchecked)
__device__ __forceinline__ mx_rec mx_clip(mx_rec r, int H, int W) {
    r.yl = min(max(r.yl, 0), H); r.yh = min(max(r.yh, 0), H);
    r.xl = min(max(r.xl, 0), W); r.xh = min(max(r.xh, 0), W);
    if (r.kind == SLAK_MIXUP_CUTMIX && (r.yl >= r.yh || r.xl >= r.xh)) r.kind = SLAK_MIXUP_NONE;
    if (r.kind != SLAK_MIXUP_CUTMIX && r.kind != SLAK_MIXUP_MIX) r.kind = SLAK_MIXUP_NONE;
    return r;
}

// the new value of one element of an image under its record, from its own original `own` and the partner's `other`; false: leave it alone
__device__ __forceinline__ bool mx_elem(const mx_rec& r, int y, int x, float own, float other, float& out) {
    if (r.kind == SLAK_MIXUP_MIX) { out = __fadd_rn(__fmul_rn(own, r.a), __fmul_rn(other, r.b)); return true; }
    if (r.kind == SLAK_MIXUP_CUTMIX && y >= r.yl && y < r.yh && x >= r.xl && x < r.xh) { out = other; return true; }
    return false;
}

__global__ __launch_bounds__(MX_T) void mixup_images_kernel(float* x, const mx_rec shared, const mx_rec* __restrict__ table, int N, int C, int H, int W) {
    const int i = blockIdx.y, j = N - 1 - i;                    // i < N / 2 <= j: never the same image
    const mx_rec ri = mx_clip(table ? table[i] : shared, H, W), rj = mx_clip(table ? table[j] : shared, H, W);
    if (ri.kind == SLAK_MIXUP_NONE && rj.kind == SLAK_MIXUP_NONE) return;
    const int HW = H * W, CHW = C * HW;
    // the pair's domain: the whole image as one row when a record is mixup, else the rows [Y0, Y1) x columns [X0, X1) of every plane that hold both boxes
    const bool full = ri.kind == SLAK_MIXUP_MIX || rj.kind == SLAK_MIXUP_MIX;
    const bool boxes = ri.kind == SLAK_MIXUP_CUTMIX || rj.kind == SLAK_MIXUP_CUTMIX;
    int Y0 = 0, Y1 = 1, X0 = 0, X1 = CHW;
    if (!full) {
        Y0 = H; Y1 = 0; X0 = W; X1 = 0;
        if (ri.kind == SLAK_MIXUP_CUTMIX) { Y0 = ri.yl; Y1 = ri.yh; X0 = ri.xl; X1 = ri.xh; }
        if (rj.kind == SLAK_MIXUP_CUTMIX) { Y0 = min(Y0, rj.yl); Y1 = max(Y1, rj.yh); X0 = min(X0, rj.xl); X1 = max(X1, rj.xh); }
    }
    const int RH = Y1 - Y0, len = X1 - X0;                      // rows per plane, floats per row; both >= 1
    const int nrows = full ? 1 : C * RH;
    const int cpr = (len + 3) / 4 + 1;                          // 16-byte pieces a row can touch, at most
    const int total = nrows * cpr;                              // <= 2 C H W: fits (MX_MAX_IMAGE)
    float* pi = x + (size_t)i * (size_t)CHW;
    float* pj = x + (size_t)j * (size_t)CHW;
    const int mis = (int)(((uintptr_t)pi >> 2) & 3u);           // floats between the 16-byte boundary below image i and its start
    const bool same = ((((uintptr_t)pi) ^ ((uintptr_t)pj)) & 15u) == 0;
    for (int t = blockIdx.x * MX_T + threadIdx.x; t < total; t += gridDim.x * MX_T) {
        const int r = t / cpr, k = t - r * cpr;
        int y = 0, off = 0;                                     // the row's first element, as an offset into the image
        if (!full) { const int c = r / RH; y = Y0 + (r - c * RH); off = (c * H + y) * W + X0; }
        const int e0 = (((mis + off) >> 2) + k) * 4 - mis;       // first element of this piece: pi + e0 is 16-byte aligned; may lie before the row
        const int lo = max(e0, off), hi = min(e0 + 4, off + len);
        if (lo >= hi) continue;
        const bool whole = hi - lo == 4;                        // then e0 >= off >= 0 and e0 + 4 <= off + len <= CHW: inside both images
        float vi[4], vj[4];
        if (whole) {
            const float4 a = *reinterpret_cast<const float4*>(pi + e0);
            vi[0] = a.x; vi[1] = a.y; vi[2] = a.z; vi[3] = a.w;
            if (same) {
                const float4 b = *reinterpret_cast<const float4*>(pj + e0);
                vj[0] = b.x; vj[1] = b.y; vj[2] = b.z; vj[3] = b.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) vj[q] = pj[e0 + q];
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool in = e0 + q >= lo && e0 + q < hi;
                vi[q] = in ? pi[e0 + q] : 0.f;
                vj[q] = in ? pj[e0 + q] : 0.f;
            }
        }
        // both originals are in registers: nothing below reads memory again
        float ni[4], nj[4];
        bool wi[4], wj[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = e0 + q;
            int ey = y, ex = X0 + (e - off);
            if (full && boxes) { const int rem = e % HW; ey = rem / W; ex = rem - ey * W; }    // a mixup image whose partner is cutmix ('elem')
            const bool in = e >= lo && e < hi;
            wi[q] = in && mx_elem(ri, ey, ex, vi[q], vj[q], ni[q]);
            wj[q] = in && mx_elem(rj, ey, ex, vj[q], vi[q], nj[q]);
        }
        if (whole && wi[0] && wi[1] && wi[2] && wi[3]) *reinterpret_cast<float4*>(pi + e0) = make_float4(ni[0], ni[1], ni[2], ni[3]);
        else {
#pragma unroll
            for (int q = 0; q < 4; ++q) if (wi[q]) pi[e0 + q] = ni[q];
        }
        if (whole && same && wj[0] && wj[1] && wj[2] && wj[3]) *reinterpret_cast<float4*>(pj + e0) = make_float4(nj[0], nj[1], nj[2], nj[3]);
        else {
#pragma unroll
            for (int q = 0; q < 4; ++q) if (wj[q]) pj[e0 + q] = nj[q];
        }
    }
}

__global__ __launch_bounds__(MX_T) void mixup_targets_kernel(const long long* __restrict__ labels, const mx_rec shared, const mx_rec* __restrict__ table,
                                                             float on, float off, float* __restrict__ out, int N, int K) {
    const int total = N * K;
    const int mis = (int)(((uintptr_t)out >> 2) & 3u);
    const int c = blockIdx.x * MX_T + threadIdx.x;              // one 16-byte piece of the flat array per thread
    const int e0 = c * 4 - mis;
    const int lo = max(e0, 0), hi = min(e0 + 4, total);
    if (lo >= hi) return;
    int n = lo / K, k = lo - n * K;
    float v[4];
    long long yn = 0, yj = 0;
    float a = 0.f, b = 0.f;
    bool fresh = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = e0 + q;
        v[q] = 0.f;
        if (e < lo || e >= hi) continue;
        if (fresh) {                                            // n < N: the labels and the record of this row and of its partner row
            yn = labels[n]; yj = labels[N - 1 - n];
            a = table ? table[n].a : shared.a; b = table ? table[n].b : shared.b;
            fresh = false;
        }
        v[q] = __fadd_rn(__fmul_rn((long long)k == yn ? on : off, a), __fmul_rn((long long)k == yj ? on : off, b));
        if (++k == K) { k = 0; ++n; fresh = true; }
    }
    if (hi - lo == 4) *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
    else {
#pragma unroll
        for (int q = 0; q < 4; ++q) if (e0 + q >= lo && e0 + q < hi) out[e0 + q] = v[q];
    }
}

static int mx_images_supported(int dt, int N, int C, int H, int W) {
    return dt == SLAK_F32 && N >= 2 && N % 2 == 0 && N <= MX_MAX_N && C >= 1 && H >= 1 && W >= 1 && (long long)C * H * W <= MX_MAX_IMAGE;
}

static int mx_targets_supported(int N, int K) { return N >= 2 && N % 2 == 0 && K >= 1 && (long long)N * K <= (1ll << 30); }

static bool mx_record_ok(const mx_rec& r, int H, int W) {
    if (r.kind != SLAK_MIXUP_NONE && r.kind != SLAK_MIXUP_MIX && r.kind != SLAK_MIXUP_CUTMIX) return false;
    return 0 <= r.yl && r.yl <= r.yh && r.yh <= H && 0 <= r.xl && r.xl <= r.xh && r.xh <= W;
}

}  // namespace slak

using namespace slak;

extern "C" {

int slak_mixup_images_supported(int x_dtype, int N, int C, int H, int W) { return mx_images_supported(x_dtype, N, C, H, W); }

int slak_mixup_images(void* x, int x_dtype, const slak_mixup_record_t* shared_host, const slak_mixup_record_t* table_dev,
                      int N, int C, int H, int W, void* stream) {
    if (!x || (shared_host == nullptr) == (table_dev == nullptr)) return SLAK_ERR_INVALID_ARG;
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || !dtype_ok(x_dtype)) return SLAK_ERR_INVALID_ARG;
    if (((uintptr_t)x % dtype_size(x_dtype)) != 0 || ((uintptr_t)table_dev & 3u) != 0) return SLAK_ERR_INVALID_ARG;
    if (shared_host && !mx_record_ok(*shared_host, H, W)) return SLAK_ERR_INVALID_ARG;
    if (!mx_images_supported(x_dtype, N, C, H, W)) return SLAK_ERR_UNSUPPORTED;
    mx_rec shared = {};
    long long pieces = ((long long)C * H * W + 3) / 4 + 1;      // per pair: the whole image ...
    if (shared_host) {
        shared = *shared_host;
        const bool empty = shared.yl == shared.yh || shared.xl == shared.xh;
        if (shared.kind == SLAK_MIXUP_NONE || (shared.kind == SLAK_MIXUP_CUTMIX && empty)) return SLAK_OK;     // every image stays as it is
        if (shared.kind == SLAK_MIXUP_CUTMIX) pieces = (long long)C * (shared.yh - shared.yl) * ((shared.xh - shared.xl + 3) / 4 + 1);   // ... or the box rows
    }
    long long gx = (pieces + MX_T * MX_PIECES - 1) / (MX_T * MX_PIECES);
    gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
    hipLaunchKernelGGL(mixup_images_kernel, dim3((unsigned)gx, (unsigned)(N / 2)), dim3(MX_T), 0, (hipStream_t)stream, (float*)x, shared, table_dev, N, C, H, W);
    SLAK_LAUNCH_CHECK();
    return SLAK_OK;
}

int slak_mixup_targets_supported(int N, int K) { return mx_targets_supported(N, K); }

int slak_mixup_targets(const long long* labels, const slak_mixup_record_t* shared_host, const slak_mixup_record_t* table_dev,
                       float on_value, float off_value, float* out, int N, int K, void* stream) {
    if (!labels || !out || (shared_host == nullptr) == (table_dev == nullptr)) return SLAK_ERR_INVALID_ARG;
    if (N <= 0 || K <= 0) return SLAK_ERR_INVALID_ARG;
    if (((uintptr_t)labels & 7u) != 0 || ((uintptr_t)out & 3u) != 0 || ((uintptr_t)table_dev & 3u) != 0) return SLAK_ERR_INVALID_ARG;
    if (!mx_targets_supported(N, K)) return SLAK_ERR_UNSUPPORTED;
    mx_rec shared = {};
    if (shared_host) shared = *shared_host;
    const long long pieces = ((long long)N * K + 3) / 4 + 1;
    hipLaunchKernelGGL(mixup_targets_kernel, dim3((unsigned)((pieces + MX_T - 1) / MX_T)), dim3(MX_T), 0, (hipStream_t)stream, labels, shared, table_dev,
                       on_value, off_value, out, N, K);
    SLAK_LAUNCH_CHECK();
    return SLAK_OK;
}

}  // extern "C"
