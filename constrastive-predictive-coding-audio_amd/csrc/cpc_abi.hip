// extern "C" boundary of libcpc_hip.so: argument checking + translation of the domain-level calls (conv / GRU / NCE /
// Adam) onto the kernel launchers.  See include/cpc_hip.h for the contract.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include "cpc_common.h"
#include "cpc_kernels.h"
#include "../../include/cpc_hip.h"

static_assert(CPC_GEMM_FORCE_GENERIC == GEMM_FORCE_GENERIC && CPC_GEMM_SMALL_TILE == GEMM_SMALL_TILE, "flag mismatch");
static_assert(CPC_GEMM_SKIP_PAD_ROWS == GEMM_SKIP_PAD_ROWS && CPC_GEMM_NO_DMA == GEMM_NO_DMA, "flag mismatch");
static_assert(CPC_GEMM_RELU == GEMM_RELU && CPC_GEMM_OUT_F32 == GEMM_OUT_F32 && CPC_GEMM_TN_NO_TR == GEMM_TN_NO_TR, "flag mismatch");
static_assert(CPC_GEMM_LINEAR_K == GEMM_LINEAR_K && CPC_GEMM_NO_PERS == GEMM_NO_PERS && CPC_GEMM_DIRECT_MASK == GEMM_DIRECT_MASK, "flag mismatch");
static_assert(CPC_GEMM_BIG_TILE == GEMM_BIG_TILE && CPC_GEMM_GENERIC_EPI == GEMM_GENERIC_EPI && CPC_GEMM_QUERY_EPI == GEMM_QUERY_EPI, "flag mismatch");
static_assert(CPC_F32 == CPC_DTYPE_F32 && CPC_BF16 == CPC_DTYPE_BF16, "dtype mismatch");

static inline int esize(int dtype) { return dtype == CPC_DTYPE_BF16 ? 2 : 4; }

extern "C" {

int cpc_abi_version(void) { return 9; }

static int gemm_nt_from_args(const cpc_gemm_nt_args* a, const void* mask_bits, float* colsum_slabs, void* stream) {
    if (!a || !a->A || !a->Bt || !a->C) return CPC_EINVAL;
    GemmNT p = {};
    p.A = a->A; p.Bt = a->Bt; p.C = a->C; p.bias = a->bias; p.mask = a->mask;
    p.mask_bits = (const unsigned char*)mask_bits; p.colsum_slabs = colsum_slabs;
    p.M = a->M; p.N = a->N; p.K = a->K;
    p.lda = a->lda; p.ldb = a->ldb; p.ldc = a->ldc;
    p.a_rpi = a->a_rpi; p.a_item = a->a_item;
    p.b_rpi = a->b_rpi; p.b_item = a->b_item;
    p.c_rpi = a->c_rpi; p.c_item = a->c_item; p.c_valid = a->c_valid;
    p.a_batch = a->a_batch; p.b_batch = a->b_batch; p.c_batch = a->c_batch;
    p.flags = a->flags;
    p.a_rpi2 = a->a_rpi2; p.a_item2 = a->a_item2; p.c_rpi2 = a->c_rpi2; p.c_item2 = a->c_item2; p.k_ranges = a->k_ranges;
    if (a->a_rpi2 && a->a_extent > 0) return CPC_EINVAL;
    if (a->k_taps < 0 || a->k_taps == 1 || (a->k_taps > 1 && (a->k_tap_stride <= 0 || a->k_tap_stride_a < 0 || a->a_extent > 0))) return CPC_EINVAL;
    if (a->k_taps == 0 && a->k_tap_stride_a) return CPC_EINVAL;      // a piece stride without pieces: refused, not ignored
    p.k_taps = a->k_taps; p.k_tap_stride = a->k_taps > 1 ? a->k_tap_stride : 0; p.k_tap_stride_a = a->k_taps > 1 ? a->k_tap_stride_a : 0;
    p.k_taps_linear = a->k_taps > 1;
    if (a->dtype == CPC_DTYPE_F32) p.flags |= GEMM_OUT_F32;
    if (a->mask && (p.flags & GEMM_OUT_F32) && a->dtype != CPC_DTYPE_F32) return CPC_EINVAL;
    // Optional extent check (see the over-read contract in cpc_hip.h): the last row of the last batch ends at ..._end elements.
    const int nb = a->batch > 0 ? a->batch : 1;
    if (a->a_extent > 0 && a->M > 0) {
        const long long last = a->a_rpi ? (long long)((a->M - 1) / a->a_rpi) * a->a_item + (long long)((a->M - 1) % a->a_rpi) * a->lda
                                        : (long long)(a->M - 1) * a->lda;
        if (last + a->K + (long long)(nb - 1) * a->a_batch > a->a_extent) return CPC_EINVAL;
    }
    if (a->b_extent > 0 && a->N > 0) {
        const long long last = a->b_rpi ? (long long)((a->N - 1) / a->b_rpi) * a->b_item + (long long)((a->N - 1) % a->b_rpi) * a->ldb
                                        : (long long)(a->N - 1) * a->ldb;
        if (last + a->K + (long long)(nb - 1) * a->b_batch > a->b_extent) return CPC_EINVAL;
    }
    return launch_gemm_nt(p, a->dtype, nb, (hipStream_t)stream);
}

int cpc_gemm_nt(const cpc_gemm_nt_args* a, void* stream) { return gemm_nt_from_args(a, nullptr, nullptr, stream); }

int cpc_gemm_nt_bits(const cpc_gemm_nt_args* a, const void* mask_bits, float* colsum_slabs, void* stream) {
    if (!mask_bits && !(a && a->mask)) return CPC_EINVAL;
    return gemm_nt_from_args(a, mask_bits, colsum_slabs, stream);
}

int cpc_gemm_nt_debug_flags(int flags) { return gemm_nt_debug_flags(flags); }

int cpc_gemm_tn(const cpc_gemm_tn_args* a, void* stream) {
    if (!a || !a->A || !a->B || !a->C) return CPC_EINVAL;
    GemmTN p;
    p.A = a->A; p.B = a->B; p.C = a->C;
    p.M = a->M; p.I = a->I; p.J = a->J;
    p.lda = a->lda; p.ldb = a->ldb; p.ldc = a->ldc;
    p.a_rpi = a->a_rpi; p.a_item = a->a_item;
    p.b_rpi = a->b_rpi; p.b_item = a->b_item;
    p.a_batch = a->a_batch; p.b_batch = a->b_batch; p.c_batch = a->c_batch;
    p.c_rpi = a->c_rpi; p.c_item = a->c_item;
    p.a_rpi2 = a->a_rpi2; p.a_item2 = a->a_item2;
    const int nsplit = a->nsplit > 0 ? a->nsplit : 1;
    p.m_chunk = nsplit > 1 ? a->m_chunk : a->M;
    p.slab_stride = a->slab_stride;
    p.flags = a->flags;
    if (a->dtype == CPC_DTYPE_F32) p.flags |= GEMM_OUT_F32;
    const int blk = a->dtype == CPC_DTYPE_BF16 ? 64 : 32;
    if (nsplit > 1 && (p.m_chunk % blk)) return CPC_EINVAL;
    return launch_gemm_tn(p, a->dtype, nsplit, a->batch > 0 ? a->batch : 1, (hipStream_t)stream);
}

int cpc_reduce_slabs(const float* slabs, float* out, int I, int J, int nslab, long long slab_stride, int cdiv, long long s_j,
                     long long s_hi, long long s_lo, void* stream) {
    if (!slabs || !out) return CPC_EINVAL;
    return launch_reduce_slabs(slabs, out, I, J, nslab, slab_stride, cdiv, s_j, s_hi, s_lo, (hipStream_t)stream);
}

int cpc_colsum(const void* X, float* slabs, int M, int N, long long ldx, int nblocks, int dtype, void* stream) {
    if (!X || !slabs) return CPC_EINVAL;
    return launch_colsum(X, slabs, M, N, ldx, dtype, nblocks, (hipStream_t)stream);
}

int cpc_conv1_fwd(const float* x, const float* w, const float* bias, void* y, int B, int C, int stride, int kw, long long ldx,
                  int L_valid, int L_alloc, int relu, int dtype, void* y_bits, void* stream) {
    if (!x || !w || !y) return CPC_EINVAL;
    if ((long long)(L_valid - 1) * stride + kw > ldx) return CPC_EINVAL;
    return launch_conv1_fwd(x, w, bias, y, B, C, stride, kw, ldx, L_valid, L_alloc, relu, dtype, (unsigned char*)y_bits, (hipStream_t)stream);
}

int cpc_conv1_fwd_rows(const float* x, const float* w, const float* bias, void* y, int B, int C, int stride, int kw, long long ldx,
                       int L_valid, int L_alloc, int relu, int dtype, void* y_bits, int row_lo, int row_hi, void* stream) {
    if (!x || !w || !y) return CPC_EINVAL;
    if ((long long)(L_valid - 1) * stride + kw > ldx) return CPC_EINVAL;
    return launch_conv1_fwd(x, w, bias, y, B, C, stride, kw, ldx, L_valid, L_alloc, relu, dtype, (unsigned char*)y_bits, (hipStream_t)stream,
                            row_lo, row_hi);
}

int cpc_sign_bits(const void* x, void* bits, long long n, int dtype, void* stream) {
    if (!x || !bits || n <= 0 || n % 32) return CPC_EINVAL;
    return launch_sign_bits(x, (unsigned char*)bits, n, dtype, (hipStream_t)stream);
}

int cpc_conv1_bwd(const float* x, const void* dy, float* slabs, int B, int C, int stride, int kw, long long ldx, int L_valid,
                  int L_alloc, int nblk_t, int nblk_b, int dtype, void* stream) {
    if (!x || !dy || !slabs) return CPC_EINVAL;
    if ((long long)(L_valid - 1) * stride + kw > ldx) return CPC_EINVAL;
    return launch_conv1_bwd(x, dy, slabs, B, C, stride, kw, ldx, L_valid, L_alloc, nblk_t, nblk_b, dtype, (hipStream_t)stream);
}

int cpc_reduce_conv_w(const float* slabs, float* out, int cin, int cout, int kw, int nslab, long long slab_stride, void* stream) {
    if (!slabs || !out) return CPC_EINVAL;
    return launch_reduce_conv_w(slabs, out, cin, cout, kw, nslab, slab_stride, (hipStream_t)stream);
}

int cpc_reduce_conv_w2d(const float* slabs, float* out, int nslab, long long slab_stride, int cout, int cin, int kh, int kw, long long s_dw,
                        long long s_dh, long long s_c, int G, long long s_g, void* stream) {
    return launch_reduce_conv_w2d(slabs, out, nslab, slab_stride, cout, cin, kh, kw, s_dw, s_dh, s_c, G, s_g, (hipStream_t)stream);
}

int cpc_conv_fwd(const void* x, const void* w_fwd, const float* bias, void* y, int B, int Cin, int Cout, int kw, int stride,
                 int Lout_alloc, int Lout_valid, int relu, long long x_tail, int dtype, void* stream) {
    if (!x || !w_fwd || !y || B <= 0 || Lout_alloc <= 0 || Lout_valid > Lout_alloc || kw <= 0 || stride <= 0) return CPC_EINVAL;
    if (x_tail < (long long)std::max(0, kw - stride) * Cin) return CPC_EINVAL;    // the last row reads kw - stride positions past the end
    GemmNT p = {};
    p.A = x; p.Bt = w_fwd; p.C = y; p.bias = bias; p.mask = nullptr;
    p.M = B * Lout_alloc; p.N = Cout; p.K = kw * Cin;
    p.lda = (long long)stride * Cin; p.ldb = p.K; p.ldc = Cout;
    p.c_rpi = Lout_alloc; p.c_item = (long long)Lout_alloc * Cout; p.c_valid = Lout_valid;
    p.flags = (relu ? GEMM_RELU : 0) | (dtype == CPC_DTYPE_F32 ? GEMM_OUT_F32 : 0);
    return launch_gemm_nt(p, dtype, 1, (hipStream_t)stream);
}

int cpc_conv_dgrad(const void* dy, const void* w_dgrad, const void* x_act, void* dx, int B, int Cin, int Cout, int kw,
                   int stride, int Lout_alloc, int Lin_valid, long long dy_head, int dtype, const void* x_act_bits, float* dx_colsum_slabs,
                   void* stream) {
    if (!dy || !w_dgrad || !dx || B <= 0 || Lout_alloc <= 0 || kw <= 0 || stride <= 0) return CPC_EINVAL;
    (void)Lin_valid;   // positions >= Lin_valid receive zeros because the pad rows of dy are zero
    const int D = (kw + stride - 1) / stride;
    if (dy_head < (long long)(D - 1) * Cout) return CPC_EINVAL;                   // the first row starts D - 1 positions before dy
    GemmNT p = {};
    p.A = (const char*)dy - (long long)(D - 1) * Cout * esize(dtype);   // D-1 zero guard rows precede the buffer
    p.Bt = w_dgrad; p.C = dx; p.bias = nullptr; p.mask = x_act;
    p.mask_bits = (const unsigned char*)x_act_bits;
    p.colsum_slabs = dx_colsum_slabs;
    p.M = B * Lout_alloc; p.N = stride * Cin; p.K = D * Cout;
    p.lda = Cout; p.ldb = p.K; p.ldc = (long long)stride * Cin;
    p.flags = dtype == CPC_DTYPE_F32 ? GEMM_OUT_F32 : 0;
    return launch_gemm_nt(p, dtype, 1, (hipStream_t)stream);
}

long long cpc_conv_dgrad_colsum_floats(int B, int Cin, int stride, int Lout_alloc) {
    return (((long long)B * Lout_alloc + 255) / 256) * stride * Cin;
}

long long cpc_conv_dgrad_conv1_floats(int B, int Cin, int stride, int Lout_alloc, int kw1, int what) {
    const long long numM = ((long long)B * Lout_alloc + 255) / 256, numN = (long long)stride * Cin / 256;
    if (what == 0) return numM * numN * (kw1 + 1) * 256;      // slabs
    return 128LL * (kw1 + 1) * Cin;                           // reduction workspace (C1F_CHUNKS partial sums)
}

int cpc_conv_dgrad_conv1(const void* dy, const void* w_dgrad, const void* x_act, const float* x, float* slabs, int B, int Cin,
                         int Cout, int kw, int stride, int Lout_alloc, long long ldx, int kw1, int stride1, int L1_valid,
                         long long dy_head, int dtype, const void* x_act_bits, void* stream) {
    if (!dy || !w_dgrad || !(x_act || x_act_bits) || !x || !slabs || B <= 0 || Lout_alloc <= 0 || dtype != CPC_DTYPE_BF16) return CPC_EINVAL;
    if (Cin % 256 || kw1 < 1 || kw1 > 15 || stride1 < 1 || L1_valid < 1 || kw <= 0 || stride <= 0) return CPC_EINVAL;
    const int D = (kw + stride - 1) / stride;
    if (dy_head < (long long)(D - 1) * Cout) return CPC_EINVAL;
    GemmNT p = {};
    p.A = (const char*)dy - (long long)(D - 1) * Cout * esize(dtype);
    p.Bt = w_dgrad; p.C = slabs /* not written */; p.bias = nullptr; p.mask = x_act;
    p.mask_bits = (const unsigned char*)x_act_bits;
    p.M = B * Lout_alloc; p.N = stride * Cin; p.K = D * Cout;
    p.lda = Cout; p.ldb = p.K; p.ldc = (long long)stride * Cin;
    p.flags = GEMM_EPI_CONV1;
    p.c1_x = x; p.c1_ldx = ldx; p.c1_slabs = slabs;
    p.c1_rpi = Lout_alloc; p.c1_sub = stride; p.c1_stride = stride1; p.c1_kw = kw1; p.c1_valid = L1_valid;
    return launch_gemm_nt(p, dtype, 1, (hipStream_t)stream);
}

int cpc_conv1_fused_reduce(const float* slabs, float* tmp, float* dw, float* db, int B, int Cin, int stride, int Lout_alloc,
                           int kw1, void* stream) {
    if (B <= 0 || Lout_alloc <= 0) return CPC_EINVAL;
    const int numM = (int)(((long long)B * Lout_alloc + 255) / 256);
    return launch_conv1_fused_reduce(slabs, tmp, dw, db, numM, Cin, stride, kw1, (hipStream_t)stream);
}

int cpc_conv_wgrad(const void* x, const void* dy, float* slabs, int B, int Cin, int Cout, int kw, int stride, int Lout_alloc,
                   int nsplit, long long x_tail, int dtype, void* stream) {
    if (!x || !dy || !slabs || B <= 0 || Lout_alloc <= 0 || nsplit <= 0 || kw <= 0 || stride <= 0) return CPC_EINVAL;
    if (x_tail < (long long)std::max(0, kw - stride) * Cin) return CPC_EINVAL;
    GemmTN p = {};
    p.A = x; p.B = dy; p.C = slabs;
    p.M = B * Lout_alloc; p.I = kw * Cin; p.J = Cout;
    p.lda = (long long)stride * Cin; p.ldb = Cout; p.ldc = Cout;
    const int blk = dtype == CPC_DTYPE_BF16 ? 64 : 32;
    int chunk = (p.M + nsplit - 1) / nsplit;
    chunk = (chunk + blk - 1) / blk * blk;
    p.m_chunk = chunk;
    p.slab_stride = (long long)p.I * p.J;
    p.flags = GEMM_OUT_F32;
    return launch_gemm_tn(p, dtype, nsplit, 1, (hipStream_t)stream);
}

// ---- the data-gradient launches on rows [row_lo, row_hi) of every item (engine.CPCEngine: the rows only the targets need are
// differentiated beside the GRU's backward recurrence).  A data-gradient GEMM row q produces input positions q s .. q s + s - 1 from output-
// gradient rows q - D + 1 .. q.
static bool rows_ok(int row_lo, int row_hi, int Lout_alloc) { return row_lo >= 0 && row_lo < row_hi && row_hi <= Lout_alloc; }

int cpc_conv_dgrad_rows(const void* dy, const void* w_dgrad, const void* x_act, void* dx, int B, int Cin, int Cout, int kw, int stride,
                        int Lout_alloc, long long dy_head, int dtype, const void* x_act_bits, float* dx_colsum_slabs, int row_lo, int row_hi,
                        void* stream) {
    if (!dy || !w_dgrad || !dx || B <= 0 || Lout_alloc <= 0 || kw <= 0 || stride <= 0 || !rows_ok(row_lo, row_hi, Lout_alloc)) return CPC_EINVAL;
    const int D = (kw + stride - 1) / stride;
    if (dy_head < (long long)(D - 1) * Cout) return CPC_EINVAL;
    const int rows = row_hi - row_lo;
    const long long es = esize(dtype), c0 = (long long)row_lo * stride * Cin;          // element offset of the first output row in dx / x_act
    GemmNT p = {};
    p.A = (const char*)dy + ((long long)row_lo - (D - 1)) * Cout * es;
    p.Bt = w_dgrad; p.C = (char*)dx + c0 * es; p.bias = nullptr;
    p.mask = x_act ? (const char*)x_act + c0 * es : nullptr;
    p.mask_bits = x_act_bits ? (const unsigned char*)x_act_bits + c0 / 8 : nullptr;
    p.colsum_slabs = dx_colsum_slabs;
    p.M = B * rows; p.N = stride * Cin; p.K = D * Cout;
    p.lda = Cout; p.ldb = p.K; p.ldc = (long long)stride * Cin;
    p.a_rpi = rows; p.a_item = (long long)Lout_alloc * Cout;
    p.c_rpi = rows; p.c_item = (long long)Lout_alloc * stride * Cin; p.c_valid = rows;
    p.flags = (dtype == CPC_DTYPE_F32 ? GEMM_OUT_F32 : 0) | (dx_colsum_slabs ? GEMM_BIG_TILE : 0);
    return launch_gemm_nt(p, dtype, 1, (hipStream_t)stream);
}

int cpc_conv_dgrad_conv1_rows(const void* dy, const void* w_dgrad, const void* x_act, const float* x, float* slabs, int B, int Cin,
                              int Cout, int kw, int stride, int Lout_alloc, long long ldx, int kw1, int stride1, int L1_valid,
                              long long dy_head, int dtype, const void* x_act_bits, int row_lo, int row_hi, void* stream) {
    if (!dy || !w_dgrad || !(x_act || x_act_bits) || !x || !slabs || B <= 0 || Lout_alloc <= 0 || dtype != CPC_DTYPE_BF16) return CPC_EINVAL;
    if (Cin % 256 || kw1 < 1 || kw1 > 15 || stride1 < 1 || L1_valid < 1 || kw <= 0 || stride <= 0 || !rows_ok(row_lo, row_hi, Lout_alloc)) return CPC_EINVAL;
    const int D = (kw + stride - 1) / stride;
    if (dy_head < (long long)(D - 1) * Cout) return CPC_EINVAL;
    const int rows = row_hi - row_lo;
    const long long es = esize(dtype), c0 = (long long)row_lo * stride * Cin;
    GemmNT p = {};
    p.A = (const char*)dy + ((long long)row_lo - (D - 1)) * Cout * es;
    p.Bt = w_dgrad; p.C = slabs /* not written */; p.bias = nullptr;
    p.mask = x_act ? (const char*)x_act + c0 * es : nullptr;
    p.mask_bits = x_act_bits ? (const unsigned char*)x_act_bits + c0 / 8 : nullptr;
    p.M = B * rows; p.N = stride * Cin; p.K = D * Cout;
    p.lda = Cout; p.ldb = p.K; p.ldc = (long long)stride * Cin;
    p.a_rpi = rows; p.a_item = (long long)Lout_alloc * Cout;
    p.c_rpi = rows; p.c_item = (long long)Lout_alloc * stride * Cin; p.c_valid = rows;
    p.flags = GEMM_EPI_CONV1 | GEMM_BIG_TILE;
    p.c1_x = x; p.c1_ldx = ldx; p.c1_slabs = slabs;
    p.c1_rpi = rows; p.c1_row0 = row_lo; p.c1_sub = stride; p.c1_stride = stride1; p.c1_kw = kw1; p.c1_valid = L1_valid;
    return launch_gemm_nt(p, dtype, 1, (hipStream_t)stream);
}

int cpc_conv1_fused_reduce_tiles(const float* slabs, float* tmp, float* dw, float* db, int num_row_tiles, int Cin, int stride, int kw1,
                                 void* stream) {
    if (num_row_tiles <= 0) return CPC_EINVAL;
    return launch_conv1_fused_reduce(slabs, tmp, dw, db, num_row_tiles, Cin, stride, kw1, (hipStream_t)stream);
}

static_assert(sizeof(cpc_conv_prep_job) == 56, "cpc_conv_prep_job layout (three pointers + eight ints)");
int cpc_conv_w_prep_plan(cpc_conv_prep_job* jobs, int njobs, int* total_blocks, int* lds_bytes) {
    return conv_w_prep_plan(jobs, njobs, total_blocks, lds_bytes);
}
int cpc_conv_w_prep_batch(const cpc_conv_prep_job* jobs_dev, int njobs, int total_blocks, int lds_bytes, int dtype, void* stream) {
    return launch_conv_w_prep_batch(jobs_dev, njobs, total_blocks, lds_bytes, dtype, (hipStream_t)stream);
}
int cpc_conv_w_prep_group(const float* w, const float* bias, void* w_fwd, void* w_dgrad, float* bias_g, int Cout, int Cin, int kh, int G,
                          int Rw, int Rd, int dtype, void* stream) {
    return launch_conv_w_prep_group(w, bias, w_fwd, w_dgrad, bias_g, Cout, Cin, kh, G, Rw, Rd, dtype, (hipStream_t)stream);
}
int cpc_conv_w_prep(const float* w, void* w_fwd, void* w_dgrad, int Cout, int Cin, int kw, int stride, int dtype, void* stream) {
    if (!w || (!w_fwd && !w_dgrad)) return CPC_EINVAL;
    return launch_conv_w_prep(w, w_fwd, w_dgrad, Cout, Cin, kw, stride, dtype, (hipStream_t)stream);
}

int cpc_maxpool_fwd(const void* in, void* out, int B, int C, int pool, int Lin_valid, int Lin_alloc, int Lout_valid, int Lout_alloc,
                    int dtype, void* stream) {
    if (!in || !out) return CPC_EINVAL;
    return launch_maxpool_fwd(in, out, B, C, pool, Lin_valid, Lin_alloc, Lout_valid, Lout_alloc, dtype, (hipStream_t)stream);
}

int cpc_maxpool_bwd(const void* in, const void* dout, void* din, int B, int C, int pool, int Lin_valid, int Lin_alloc, int Lout_alloc,
                    int dtype, void* stream) {
    if (!in || !dout || !din) return CPC_EINVAL;
    return launch_maxpool_bwd(in, dout, din, B, C, pool, Lin_valid, Lin_alloc, Lout_alloc, dtype, (hipStream_t)stream);
}

int cpc_relu_row_bwd(const float* dc, const void* y, void* dy, int B, int C, long long item_stride, long long row_off, int dtype,
                     void* stream) {
    if (!dc || !y || !dy) return CPC_EINVAL;
    return launch_relu_row_bwd(dc, y, dy, B, C, item_stride, row_off, dtype, (hipStream_t)stream);
}

int cpc_pe_scale_fwd(const void* top, const float* pe, void* x0, int B, int S, int C, long long item_stride, float scale,
                     int dtype, void* stream) {
    if (!top || !pe || !x0) return CPC_EINVAL;
    return launch_pe_scale_fwd(top, pe, x0, B, S, C, item_stride, scale, dtype, (hipStream_t)stream);
}

int cpc_pe_scale_bwd(const void* g1, const void* g2, void* dtop, int B, int S, int C, long long item_stride, float scale,
                     int dtype, void* stream) {
    if (!g1 || !dtop) return CPC_EINVAL;
    return launch_pe_scale_bwd(g1, g2, dtop, B, S, C, item_stride, scale, dtype, (hipStream_t)stream);
}

int cpc_attn_fwd(const void* qkv, void* out, void* P, int B, int S, int C, int heads, float drop_p, unsigned long long seed,
                 unsigned site, int dtype, void* stream) {
    if (!qkv || !out || !P) return CPC_EINVAL;
    return launch_attn_fwd(qkv, out, P, B, S, C, heads, drop_p, seed, site, dtype, (hipStream_t)stream);
}

int cpc_attn_bwd(const void* qkv, const void* P, const void* dout, void* dqkv, int B, int S, int C, int heads, float drop_p,
                 unsigned long long seed, unsigned site, int dtype, void* stream) {
    if (!qkv || !P || !dout || !dqkv) return CPC_EINVAL;
    return launch_attn_bwd(qkv, P, dout, dqkv, B, S, C, heads, drop_p, seed, site, dtype, (hipStream_t)stream);
}

int cpc_add_ln_fwd(const void* a, const void* b, const float* w, const float* bias, void* r_out, void* y, float* stats, int M,
                   int C, float eps, float drop_p, unsigned long long seed, unsigned site, int dtype, void* stream) {
    if (!a || !y || !stats) return CPC_EINVAL;
    return launch_add_ln_fwd(a, b, w, bias, r_out, y, stats, M, C, eps, drop_p, seed, site, dtype, (hipStream_t)stream);
}

int cpc_ln_bwd(const void* g1, const void* g2, const void* r, const float* stats, const float* w, void* dr, float* slabs, int M,
               int C, int bcast, float gscale, int nblocks, void* dr_b, float drop_p, unsigned long long seed, unsigned site,
               int dtype, void* stream) {
    if (!g1 || !r || !stats || !w || !dr || !slabs) return CPC_EINVAL;
    return launch_ln_bwd(g1, g2, r, stats, w, dr, slabs, M, C, bcast, gscale, nblocks, dr_b, drop_p, seed, site, dtype,
                         (hipStream_t)stream);
}

int cpc_ln_tangent(const float* at, const float* bt, const float* r, const float* stats, const float* w, float* rt_out, float* yt,
                   int M, int C, float drop_p, unsigned long long seed, unsigned site, void* stream) {
    if (!at || !r || !stats || !w || !yt) return CPC_EINVAL;
    return launch_ln_tangent(at, bt, r, stats, w, rt_out, yt, M, C, drop_p, seed, site, (hipStream_t)stream);
}

int cpc_ln_gp(const float* g1, const float* g2, const float* rt, const float* r, const float* stats, const float* w, float* dr,
              float* dr_b, float* slabs, int M, int C, int bcast, float gscale, int nblocks, float drop_p, unsigned long long seed,
              unsigned site, void* stream) {
    if (!g1 || !rt || !r || !stats || !w || !dr || !slabs) return CPC_EINVAL;
    return launch_ln_gp(g1, g2, rt, r, stats, w, dr, dr_b, slabs, M, C, bcast, gscale, nblocks, drop_p, seed, site, (hipStream_t)stream);
}

int cpc_attn_tangent(const float* qkv, const float* qkvt, const float* P, float* out_t, int B, int S, int C, int heads, float drop_p,
                     unsigned long long seed, unsigned site, void* stream) {
    if (!qkv || !qkvt || !P || !out_t) return CPC_EINVAL;
    return launch_attn_tangent(qkv, qkvt, P, out_t, B, S, C, heads, drop_p, seed, site, (hipStream_t)stream);
}

int cpc_attn_gp(const float* qkv, const float* qkvt, const float* P, const float* dout, float* dqkv, int B, int S, int C, int heads,
                float drop_p, unsigned long long seed, unsigned site, void* stream) {
    if (!qkv || !qkvt || !P || !dout || !dqkv) return CPC_EINVAL;
    return launch_attn_gp(qkv, qkvt, P, dout, dqkv, B, S, C, heads, drop_p, seed, site, (hipStream_t)stream);
}

int cpc_attn128_fwd(const void* qkv, void* out, void* P, int B, int S, int C, int heads, float drop_p, unsigned long long seed,
                    unsigned site, int dtype, void* stream) {
    if (!qkv || !out || !P) return CPC_EINVAL;
    return launch_attn128_fwd(qkv, out, P, B, S, C, heads, drop_p, seed, site, dtype, (hipStream_t)stream);
}

int cpc_attn128_bwd(const void* qkv, const void* P, const void* dout, void* dqkv, int B, int S, int C, int heads, float drop_p,
                    unsigned long long seed, unsigned site, int dtype, void* stream) {
    if (!qkv || !P || !dout || !dqkv) return CPC_EINVAL;
    return launch_attn128_bwd(qkv, P, dout, dqkv, B, S, C, heads, drop_p, seed, site, dtype, (hipStream_t)stream);
}

int cpc_attn128_tangent(const float* qkv, const float* qkvt, const float* P, float* out_t, int B, int S, int C, int heads, float drop_p,
                        unsigned long long seed, unsigned site, void* stream) {
    if (!qkv || !qkvt || !P || !out_t) return CPC_EINVAL;
    return launch_attn128_tangent(qkv, qkvt, P, out_t, B, S, C, heads, drop_p, seed, site, (hipStream_t)stream);
}

int cpc_attn128_gp(const float* qkv, const float* qkvt, const float* P, const float* dout, float* dqkv, int B, int S, int C, int heads,
                   float drop_p, unsigned long long seed, unsigned site, void* stream) {
    if (!qkv || !qkvt || !P || !dout || !dqkv) return CPC_EINVAL;
    return launch_attn128_gp(qkv, qkvt, P, dout, dqkv, B, S, C, heads, drop_p, seed, site, (hipStream_t)stream);
}

int cpc_dropout(void* x, long long n, float drop_p, unsigned long long seed, unsigned site, int dtype, void* stream) {
    if (!x) return CPC_EINVAL;
    return launch_dropout(x, n, drop_p, seed, site, dtype, (hipStream_t)stream);
}

int cpc_dropout_mask(float* mask, long long n, float drop_p, unsigned long long seed, unsigned site, void* stream) {
    if (!mask) return CPC_EINVAL;
    return launch_dropout_mask(mask, n, drop_p, seed, site, (hipStream_t)stream);
}

int cpc_mean_time(const void* x, void* out, int B, int S, int C, int dtype, void* stream) {
    if (!x || !out) return CPC_EINVAL;
    return launch_mean_time(x, out, B, S, C, dtype, (hipStream_t)stream);
}

int cpc_scalogram_pointwise(const float* cq, const float* fixed_pd, const float* pd_scale, float* out, int B, int Tn, int bins,
                            long long ldq, int phase, float offset, float log_offset, float norm, float power, int ph, int pw,
                            void* stream) {
    if (!cq || !out) return CPC_EINVAL;
    return launch_scalogram_pointwise(cq, fixed_pd, pd_scale, out, B, Tn, bins, ldq, phase, offset, log_offset, norm, power, ph, pw,
                                      (hipStream_t)stream);
}

int cpc_im2col2d(const void* in, void* col, const int* grid, int kh, int kw, int sh, int sw, int ph, int pw, int Ho, int Wo, int Kp,
                 int in_f32, int dtype, void* stream) {
    if (!in || !col) return CPC_EINVAL;
    return launch_im2col2d(in, col, grid, kh, kw, sh, sw, ph, pw, Ho, Wo, Kp, in_f32, dtype, (hipStream_t)stream);
}

int cpc_col2im2d(const void* dcol, void* din, const int* grid, int kh, int kw, int sh, int sw, int ph, int pw, int Ho, int Wo, int Kp,
                 int accumulate, int dtype, void* stream) {
    if (!dcol || !din) return CPC_EINVAL;
    return launch_col2im2d(dcol, din, grid, kh, kw, sh, sw, ph, pw, Ho, Wo, Kp, accumulate, dtype, (hipStream_t)stream);
}

int cpc_dw_fwd(const void* col, const float* w, void* y, long long M, int C, int taps, int Kp, int rpi, long long item, int dtype,
               void* stream) {
    if (!col || !w || !y) return CPC_EINVAL;
    return launch_dw_fwd(col, w, y, M, C, taps, Kp, rpi, item, dtype, (hipStream_t)stream);
}
int cpc_dw_bwd_col(const void* dy, const float* w, void* dcol, long long M, int C, int taps, int Kp, int rpi, long long item, int dtype,
                   void* stream) {
    if (!dy || !w || !dcol) return CPC_EINVAL;
    return launch_dw_bwd_col(dy, w, dcol, M, C, taps, Kp, rpi, item, dtype, (hipStream_t)stream);
}
int cpc_dw_bwd_w(const void* col, const void* dy, float* slabs, long long M, int C, int taps, int Kp, int rpi, long long item,
                 int nblocks, int dtype, void* stream) {
    if (!col || !dy || !slabs) return CPC_EINVAL;
    return launch_dw_bwd_w(col, dy, slabs, M, C, taps, Kp, rpi, item, nblocks, dtype, (hipStream_t)stream);
}

int cpc_bn_stats(const void* x, float* slabs, long long rows, int C, int nblocks, int dtype, void* stream) {
    if (!x || !slabs) return CPC_EINVAL;
    return launch_bn_stats(x, slabs, rows, C, nblocks, dtype, (hipStream_t)stream);
}

int cpc_bn_finalize(const float* slabs, int nslab, int C, double count, float eps, float momentum, float* stats, float* run_mean,
                    float* run_var, void* stream) {
    if (!slabs || !stats) return CPC_EINVAL;
    return launch_bn_finalize(slabs, nslab, C, count, eps, momentum, stats, run_mean, run_var, (hipStream_t)stream);
}

int cpc_bn_apply_residual(const void* x, const int* gx, const void* res, const int* gr, void* out, const int* go, const float* stats,
                          const float* gamma, const float* beta, int oh, int ow, int relu_in, int relu_out, int r_f32, unsigned char* bits,
                          const int* ga, unsigned char* obits, int dtype, void* stream) {
    return launch_bn_apply_residual(x, gx, res, gr, out, go, stats, gamma, beta, oh, ow, relu_in, relu_out, r_f32, bits, ga, dtype, (hipStream_t)stream,
                                    obits);
}
int cpc_bn_bwd_reduce_res(const void* dout, const int* gd, const unsigned char* obits, const unsigned char* abits, const int* ga, const void* x,
                          const int* gx, const float* stats, float* slabs, int nblocks, int dtype, void* stream) {
    return launch_bn_bwd_reduce_res(dout, gd, obits, abits, ga, x, gx, stats, slabs, nblocks, dtype, (hipStream_t)stream);
}
int cpc_bn_bwd_apply_res(const void* dout, const int* gd, const unsigned char* obits, const unsigned char* abits, const int* ga, const void* x,
                         void* dx, const int* gx, const float* stats, const float* gamma, const float* dgamma, const float* dbeta, double count,
                         int train, void* dres, const int* gr, int oh, int ow, int dtype, void* stream) {
    return launch_bn_bwd_apply_res(dout, gd, obits, abits, ga, x, dx, gx, stats, gamma, dgamma, dbeta, count, train, dres, gr, oh, ow, dtype,
                                   (hipStream_t)stream);
}
int cpc_bn_apply(const void* x, const int* gx, void* out, const int* go, const float* stats, const float* gamma, const float* beta,
                 int relu, int x_f32, int dtype, void* stream) {
    if (!x || !out || !stats || !gamma || !beta) return CPC_EINVAL;
    return launch_bn_apply(x, gx, out, go, stats, gamma, beta, relu, x_f32, dtype, (hipStream_t)stream);
}

int cpc_bn_bwd_reduce(const void* dy, const void* y, const int* gy, const void* x, const int* gx, const float* stats, float* slabs,
                      int relu, int nblocks, int x_f32, int dtype, void* stream) {
    if (!dy || !x || !stats || !slabs || (relu && !y)) return CPC_EINVAL;
    return launch_bn_bwd_reduce(dy, y, gy, x, gx, stats, slabs, relu, nblocks, x_f32, dtype, (hipStream_t)stream);
}

int cpc_bn_bwd_apply(const void* dy, const void* y, const int* gy, const void* x, void* dx, const int* gx, const float* stats,
                     const float* gamma, const float* dgamma, const float* dbeta, double count, int relu, int train, int x_f32,
                     int dtype, void* stream) {
    if (!dy || !x || !dx || !stats || !gamma || (relu && !y)) return CPC_EINVAL;
    return launch_bn_bwd_apply(dy, y, gy, x, dx, gx, stats, gamma, dgamma, dbeta, count, relu, train, x_f32, dtype, (hipStream_t)stream);
}

int cpc_maxpool2d_fwd(const void* in, const int* gi, void* out, const int* go, int p, int in_f32, int dtype, void* stream) {
    if (!in || !out) return CPC_EINVAL;
    return launch_maxpool2d_fwd(in, gi, out, go, p, in_f32, dtype, (hipStream_t)stream);
}

int cpc_maxpool2d_bwd(const void* in, void* din, const int* gi, const void* dout, const int* go, int p, int accumulate, int dtype,
                      void* stream) {
    if (!in || !din || !dout) return CPC_EINVAL;
    return launch_maxpool2d_bwd(in, din, gi, dout, go, p, accumulate, dtype, (hipStream_t)stream);
}

int cpc_residual_add(const void* a, const int* ga, const void* r, const int* gr, void* out, const int* go, int oh, int ow, int relu,
                     int r_f32, int dtype, void* stream) {
    if (!a || !r || !out) return CPC_EINVAL;
    return launch_residual_add(a, ga, r, gr, out, go, oh, ow, relu, r_f32, dtype, (hipStream_t)stream);
}

int cpc_residual_add_bwd(const void* dout, const void* out, const int* go, void* da, const int* ga, void* dr, const int* gr, int oh,
                         int ow, int relu, int r_f32, int dtype, void* stream) {
    if (!dout || !da || !dr || (relu && !out)) return CPC_EINVAL;
    return launch_residual_add_bwd(dout, out, go, da, ga, dr, gr, oh, ow, relu, r_f32, dtype, (hipStream_t)stream);
}

int cpc_stem_supported(int cin, int cout, int kh, int kw, int sh, int hin, int ph) { return launch_stem_supported(cin, cout, kh, kw, sh, hin, ph); }

int cpc_stem_stats(const float* x, const int* gx, const float* w, const float* bias, const int* conv, float* slabs, int nblocks,
                   void* stream) {
    if (!x || !gx || !w || !conv || !slabs) return CPC_EINVAL;
    return launch_stem_stats(x, gx, w, bias, conv[0], conv[1], conv[2], conv[3], conv[4], conv[5], conv[6], conv[7], conv[8], slabs, nblocks,
                             (hipStream_t)stream);
}

int cpc_stem_apply(const float* x, const int* gx, const float* w, const float* bias, const int* conv, const float* stats,
                   const float* gamma, const float* beta, void* out, const int* go, int nblocks, int dtype, void* stream) {
    if (!x || !gx || !w || !conv || !stats || !gamma || !beta || !out || !go) return CPC_EINVAL;
    return launch_stem_apply(x, gx, w, bias, conv[0], conv[1], conv[2], conv[3], conv[4], conv[5], conv[6], conv[7], conv[8], stats, gamma, beta,
                             out, go, nblocks, dtype, (hipStream_t)stream);
}

int cpc_stem_bwd_reduce(const float* x, const int* gx, const float* w, const float* bias, const int* conv, const float* stats,
                        const void* da, const void* a, const int* ga, float* slabs, int nblocks, int dtype, void* stream) {
    if (!x || !gx || !w || !conv || !stats || !da || !a || !ga || !slabs) return CPC_EINVAL;
    return launch_stem_bwd_reduce(x, gx, w, bias, conv[0], conv[1], conv[2], conv[3], conv[4], conv[5], conv[6], conv[7], conv[8], stats, da, a,
                                  ga, slabs, nblocks, dtype, (hipStream_t)stream);
}

int cpc_stem_bwd_wgrad(const float* x, const int* gx, const float* w, const float* bias, const int* conv, const float* stats,
                       const float* gamma, const float* dgamma, const float* dbeta, double count, const void* da, const void* a,
                       const int* ga, float* slabs, int nblocks, int dtype, void* stream) {
    if (!x || !gx || !w || !conv || !stats || !gamma || !dgamma || !dbeta || !da || !a || !ga || !slabs) return CPC_EINVAL;
    return launch_stem_bwd_wgrad(x, gx, w, bias, conv[0], conv[1], conv[2], conv[3], conv[4], conv[5], conv[6], conv[7], conv[8], stats, gamma,
                                 dgamma, dbeta, count, da, a, ga, slabs, nblocks, dtype, (hipStream_t)stream);
}

int cpc_stem_residual_bn_add(const void* y, const int* gy, const float* xp, const int* gp, const float* wr, void* out, const int* go, int oh, int ow,
                             int relu, const float* stats, const float* gamma, const float* beta, unsigned char* bits, const int* ga,
                             unsigned char* obits, int dtype, void* stream) {
    if (!y || !xp || !wr || !out) return CPC_EINVAL;
    return launch_stem_residual_bn_add(y, gy, xp, gp, wr, out, go, oh, ow, relu, stats, gamma, beta, bits, ga, dtype, (hipStream_t)stream, obits);
}
int cpc_stem_residual_wgrad_bits(const void* dout, const unsigned char* obits, const int* go, const int* gm, const float* xp, const int* gp,
                                 float* slabs, int oh, int ow, int nblocks, int dtype, void* stream) {
    if (!dout || !obits || !go || !gm || !xp || !gp || !slabs) return CPC_EINVAL;
    return launch_stem_residual_bwd(dout, nullptr, go, nullptr, gm, xp, gp, slabs, oh, ow, 1, nblocks, dtype, (hipStream_t)stream, obits);
}
int cpc_stem_residual_add(const void* main_, const int* gm, const float* xp, const int* gp, const float* wr, void* out, const int* go,
                          int oh, int ow, int relu, int dtype, void* stream) {
    if (!main_ || !gm || !xp || !gp || !wr || !out || !go) return CPC_EINVAL;
    return launch_stem_residual_add(main_, gm, xp, gp, wr, out, go, oh, ow, relu, dtype, (hipStream_t)stream);
}

int cpc_stem_residual_bwd(const void* dout, const void* out, const int* go, void* dmain, const int* gm, const float* xp, const int* gp,
                          float* slabs, int oh, int ow, int relu, int nblocks, int dtype, void* stream) {
    if (!dout || !go || !dmain || !gm || !xp || !gp || !slabs || (relu && !out)) return CPC_EINVAL;
    return launch_stem_residual_bwd(dout, out, go, dmain, gm, xp, gp, slabs, oh, ow, relu, nblocks, dtype, (hipStream_t)stream);
}

int cpc_bn_apply_bits(const void* x, const int* gx, void* out, const int* go, const float* stats, const float* gamma, const float* beta,
                      int relu, void* out_bits, int dtype, void* stream) {
    if (!x || !out || !stats || !gamma || !beta || !out_bits) return CPC_EINVAL;
    return launch_bn_apply(x, gx, out, go, stats, gamma, beta, relu, 0, dtype, (hipStream_t)stream, (unsigned char*)out_bits);
}

int cpc_bn_bwd_reduce_bits(const void* dy, const void* y_bits, const int* gy, const void* x, const int* gx, const float* stats,
                           float* slabs, int nblocks, int dtype, void* stream) {
    if (!dy || !y_bits || !x || !stats || !slabs) return CPC_EINVAL;
    return launch_bn_bwd_reduce(dy, nullptr, gy, x, gx, stats, slabs, 1, nblocks, 0, dtype, (hipStream_t)stream, (const unsigned char*)y_bits);
}

int cpc_bn_bwd_apply_bits(const void* dy, const void* y_bits, const int* gy, const void* x, void* dx, const int* gx, const float* stats,
                          const float* gamma, const float* dgamma, const float* dbeta, double count, int train, int dtype, void* stream) {
    if (!dy || !y_bits || !x || !dx || !stats || !gamma) return CPC_EINVAL;
    return launch_bn_bwd_apply(dy, nullptr, gy, x, dx, gx, stats, gamma, dgamma, dbeta, count, 1, train, 0, dtype, (hipStream_t)stream,
                               (const unsigned char*)y_bits);
}

int cpc_maxpool2d_select(const void* in, const void* sel, const int* gi, void* out, const int* go, int p, int in_f32, int dtype,
                         void* stream) {
    if (!in || !sel || !out) return CPC_EINVAL;
    return launch_maxpool2d_select(in, sel, gi, out, go, p, in_f32, dtype, (hipStream_t)stream);
}

int cpc_gp_direction(const float* g, float* v, long long npix, int C, float factor, float* partial, int nblocks, void* stream) {
    if (!g || !v || !partial) return CPC_EINVAL;
    return launch_gp_direction(g, v, npix, C, factor, partial, nblocks, (hipStream_t)stream);
}

int cpc_bn_gp_cross(const void* x, const void* yt, const void* delta, void* out, const int* gx, const float* stats, const float* coef,
                    int x_f32, int dtype, void* stream) {
    if (!x || !yt || !delta || !out || !stats || !coef) return CPC_EINVAL;
    return launch_bn_gp_cross(x, yt, delta, out, gx, stats, coef, x_f32, dtype, (hipStream_t)stream);
}

int cpc_relu_mask(void* g, const void* y, long long n, int dtype, void* stream) {
    if (!g || !y) return CPC_EINVAL;
    return launch_relu_mask(g, y, n, dtype, (hipStream_t)stream);
}

int cpc_accumulate(void* a, const void* b, long long n, int dtype, void* stream) {
    if (!a || !b) return CPC_EINVAL;
    return launch_accumulate(a, b, n, dtype, (hipStream_t)stream);
}

int cpc_split3_bf16(const float* src, void* dst, long long n, void* stream) {
    if (!src || !dst) return CPC_EINVAL;
    return launch_split3_bf16(src, dst, n, (hipStream_t)stream);
}

int cpc_adam_dev(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2, float eps, float* state,
                 float grad_scale, const float* skip, void* stream) {
    return launch_adam_dev({p, g, m, v, n, lr, b1, b2, eps, grad_scale, skip, nullptr, 0.f, nullptr, 0}, state, false, 0, 0, 0, 0.f, 0,
                           (hipStream_t)stream);
}

int cpc_cast2d(const float* src, void* dst, int R, int C, long long sr, long long sc, int dtype, void* stream) {
    if (!src || !dst) return CPC_EINVAL;
    return launch_cast2d(src, dst, R, C, sr, sc, dtype, (hipStream_t)stream);
}

int cpc_cast2d_batch(const void* jobs, int njobs, int dtype, void* stream) {
    return launch_cast2d_batch(jobs, njobs, dtype, (hipStream_t)stream);
}

int cpc_prep_frag(const float* src, void* dst, int R, int Kd, long long ld, int transpose, int dtype, void* stream) {
    if (!src || !dst) return CPC_EINVAL;
    return launch_prep_frag(src, dst, R, Kd, ld, transpose, dtype, (hipStream_t)stream);
}

long long cpc_gru_tape_elems(int B, int V, int H, int dtype) { return gru_tape_elems(B, V, H, dtype); }

int cpc_gru_fwd(const void* Gi, const void* Wfrag, const float* bhh, void* Hall, void* tape, float* c_out, int B, int V,
                int H, int dtype, void* stream) {
    if (!Gi || !Wfrag || !Hall || !tape || !c_out) return CPC_EINVAL;
    return launch_gru_fwd(Gi, Wfrag, bhh, Hall, tape, c_out, B, V, H, dtype, (hipStream_t)stream);
}

int cpc_gru_fwd_h0(const void* Gi, const void* Wfrag, const float* bhh, const float* h0, void* Hall, void* tape, float* c_out, int B,
                   int V, int H, int dtype, void* stream) {
    if (!Gi || !Wfrag || !Hall || !tape || !c_out) return CPC_EINVAL;
    return launch_gru_fwd(Gi, Wfrag, bhh, Hall, tape, c_out, B, V, H, dtype, (hipStream_t)stream, h0);
}

int cpc_gru_bwd(const float* dc, const void* tape, const void* WTfrag, void* dG, int B, int V, int H, int dtype, void* stream) {
    if (!dc || !tape || !WTfrag || !dG) return CPC_EINVAL;
    return launch_gru_bwd(dc, tape, WTfrag, dG, B, V, H, dtype, (hipStream_t)stream);
}

int cpc_gru_bwd_steps(const float* dc, const void* dHs, long long ld_h, const void* tape, const void* WTfrag, void* dG, int B, int V,
                      int H, int dtype, void* stream) {
    if (!tape || !WTfrag || !dG || (!dc && !dHs)) return CPC_EINVAL;
    return launch_gru_bwd(dc, tape, WTfrag, dG, B, V, H, dtype, (hipStream_t)stream, dHs, ld_h);
}

int cpc_gru_gp_fwd(const float* Gi, const float* GiT, const float* WT, const float* bhh, float* tape, float* ct_out, int B,
                   int V, int H, void* stream) {
    if (!Gi || !GiT || !WT || !bhh || !tape || !ct_out) return CPC_EINVAL;
    return launch_gru_gp_fwd(Gi, GiT, WT, bhh, tape, ct_out, B, V, H, (hipStream_t)stream);
}

int cpc_gru_gp_bwd(const float* dc, const float* tape, const float* W, float* dA, int B, int V, int H, void* stream) {
    if (!dc || !tape || !W || !dA) return CPC_EINVAL;
    return launch_gru_gp_bwd(dc, tape, W, dA, B, V, H, (hipStream_t)stream);
}

long long cpc_lstm_tape_elems(int B, int V, int H, int dtype) { return lstm_tape_elems(B, V, H, dtype); }

int cpc_lstm_fwd(const void* Gi, const void* Wfrag, const float* bhh, const float* h0, const float* c0, void* Hall, void* tape,
                 float* h_out, float* cell_out, int B, int V, int H, int dtype, void* stream) {
    if (!Gi || !Wfrag || !Hall || !tape || !h_out || !cell_out) return CPC_EINVAL;
    return launch_lstm_fwd(Gi, Wfrag, bhh, h0, c0, Hall, tape, h_out, cell_out, B, V, H, dtype, (hipStream_t)stream);
}

int cpc_lstm_bwd(const float* dh_last, const void* tape, const void* WTfrag, void* dG, int B, int V, int H, int dtype, void* stream) {
    if (!dh_last || !tape || !WTfrag || !dG) return CPC_EINVAL;
    return launch_lstm_bwd(dh_last, tape, WTfrag, dG, B, V, H, dtype, (hipStream_t)stream);
}

int cpc_lstm_bwd_steps(const float* dh_last, const void* dHs, long long ld_h, const void* tape, const void* WTfrag, void* dG, int B,
                       int V, int H, int dtype, void* stream) {
    if (!tape || !WTfrag || !dG || (!dh_last && !dHs)) return CPC_EINVAL;
    return launch_lstm_bwd(dh_last, tape, WTfrag, dG, B, V, H, dtype, (hipStream_t)stream, dHs, ld_h);
}

int cpc_anchor_target_grad(const float* dT, void* dtop, long long item_stride, int A, int B, int K, int E, int first_row, int stride,
                           int row_lo, int row_hi, int accumulate, int dtype, void* stream) {
    if (!dT || !dtop) return CPC_EINVAL;
    return launch_anchor_target_grad(dT, dtop, item_stride, A, B, K, E, first_row, stride, row_lo, row_hi, accumulate, dtype,
                                     (hipStream_t)stream);
}

extern int g_gru_force_streaming;
int cpc_gru_set_streaming(int on) {
    const int old = g_gru_force_streaming;
    g_gru_force_streaming = on ? 1 : 0;
    return old;
}

long long cpc_nce_workspace_floats(int B, int K) { return nce_workspace_floats(B, K); }

int cpc_nce_loss(const float* S, void* dS, void* dST, float* out, float* workspace, int B, int K, int ld, int softplus,
                 float regularization, int dtype, void* stream) {
    if (!S || !dS || !dST || !out || !workspace) return CPC_EINVAL;
    return launch_nce(S, dS, dST, out, workspace, B, K, ld, softplus, regularization, dtype, (hipStream_t)stream);
}

long long cpc_nce_sampled_workspace_floats(int B, int K) { return nce_sampled_workspace_floats(B, K); }

int cpc_nce_loss_sampled(const float* S, void* dS, void* dST, float* out, float* workspace, int B, int K, int ld, int softplus,
                         float regularization, int n_neg, unsigned long long seed, unsigned long long draw, int dtype, void* stream) {
    if (!S || !dS || !dST || !out || !workspace) return CPC_EINVAL;
    return launch_nce_sampled(S, dS, dST, out, workspace, B, K, ld, softplus, regularization, n_neg, seed, draw, dtype, (hipStream_t)stream);
}

int cpc_nce_sample_mask(unsigned char* mask, int B, int K, int n_neg, unsigned long long seed, unsigned long long draw, void* stream) {
    return launch_nce_sample_mask(mask, B, K, n_neg, seed, draw, (hipStream_t)stream);
}

long long cpc_nce_grouped_workspace_floats(int B, int K) { return nce_grouped_workspace_floats(B, K); }

int cpc_nce_loss_grouped(const float* S, void* dS, void* dST, float* out, float* workspace, int B, int K, int ld, int softplus,
                         float regularization, const int* groups, int mode, int n_neg, unsigned long long seed, unsigned long long draw,
                         int dtype, void* stream) {
    if (!S || !dS || !dST || !out || !workspace || !groups) return CPC_EINVAL;
    return launch_nce_grouped(S, dS, dST, out, workspace, B, K, ld, softplus, regularization, groups, mode, n_neg, seed, draw, dtype,
                              (hipStream_t)stream);
}

int cpc_nce_group_mask(unsigned char* mask, const int* groups, int B, int K, int mode, int n_neg, unsigned long long seed,
                       unsigned long long draw, void* stream) {
    return launch_nce_group_mask(mask, groups, B, K, mode, n_neg, seed, draw, (hipStream_t)stream);
}

long long cpc_nce_banked_workspace_floats(int B, int K, int slots) { return nce_banked_workspace_floats(B, K, slots); }

int cpc_nce_loss_banked(const float* S, void* dS, void* dST_cur, float* out, float* workspace, int B, int K, int ld, int slots, int cur,
                        unsigned long long valid_mask, int softplus, float regularization, int dtype, void* stream) {
    if (!S || !dS || !dST_cur || !out || !workspace) return CPC_EINVAL;
    return launch_nce_banked(S, dS, dST_cur, out, workspace, B, K, ld, slots, cur, valid_mask, softplus, regularization, dtype,
                             (hipStream_t)stream);
}

int cpc_gp_score_coeff(const float* S, const float* St1, const float* St2, float* W, float* WT, int nmat, int rows, int cols, int ld,
                       int ldT, int mode, void* stream) {
    if (!S || !W || !WT) return CPC_EINVAL;
    return launch_gp_score_coeff(S, St1, St2, W, WT, nmat, rows, cols, ld, ldT, mode, (hipStream_t)stream);
}

long long cpc_nce_all_workspace_floats(int B, int K) { return nce_all_workspace_floats(B, K); }

int cpc_nce_loss_all(const float* S, const float* ST, void* dS, void* dST, float* out, float* workspace, int B, int K, int ld,
                     int softplus, float regularization, int dtype, void* stream) {
    if (!S || !ST || !dS || !dST || !out || !workspace) return CPC_EINVAL;
    return launch_nce_all(S, ST, dS, dST, out, workspace, B, K, ld, softplus, regularization, dtype, (hipStream_t)stream);
}

int cpc_score_lse(const void* P, const void* T, float* S, float* pm, float* ps, float* valid, int M, int N, int E, long long ldp,
                  long long ldt, long long lds, int diag_off, void* stream) {
    return launch_score_lse(P, T, S, pm, ps, valid, M, N, E, ldp, ldt, lds, diag_off, (hipStream_t)stream);
}

int cpc_nce_lse_merge(const float* pm, const float* ps, int nparts, int ncols, int softplus, float nrows_total, float* lse, float* colp,
                      void* stream) {
    return launch_nce_lse_merge(pm, ps, nparts, ncols, softplus, nrows_total, lse, colp, (hipStream_t)stream);
}

long long cpc_nce_fused_grad_blocks(int items, int ncols) { return nce_fused_grad_blocks(items, ncols); }

int cpc_nce_fused_grad(const float* S, const float* lse, void* dS, void* dST, float* gradp, int items, int K, int ncols, long long ld,
                       long long ldT, int diag_off, int softplus, float regularization, float n_rows_total, float n_items_total, void* stream) {
    return launch_nce_fused_grad(S, lse, dS, dST, gradp, items, K, ncols, ld, ldT, diag_off, softplus, regularization, n_rows_total,
                                 n_items_total, (hipStream_t)stream);
}

int cpc_nce_fused_finalize(const float* colp, int ncolp, const float* valid, int nvalid, const float* gradp, int ngrad, float* sums, int mode,
                           float n_rows_total, float n_items_total, int K, float regularization, int softplus, float* out, void* stream) {
    return launch_nce_fused_finalize(colp, ncolp, valid, nvalid, gradp, ngrad, sums, mode, n_rows_total, n_items_total, K, regularization,
                                     softplus, out, (hipStream_t)stream);
}

long long cpc_nce_eval_workspace_floats(int B, int K) { return nce_eval_workspace_floats(B, K); }

int cpc_nce_eval(const float* S, float* out, float* workspace, int B, int K, int ld, int softplus, int all_timesteps, int accumulate,
                 void* stream) {
    if (!S || !out || !workspace) return CPC_EINVAL;
    return launch_nce_eval(S, out, workspace, B, K, ld, softplus, all_timesteps, accumulate, (hipStream_t)stream);
}

int cpc_diff_scores(const void* P, const void* T, float* S, float* ST, int M, int N, int E, long long ldp, long long ldt, int t_rpi,
                    long long t_item, long long p_batch, long long t_batch, long long s_batch, int batch, int lds, int dtype, void* stream) {
    if (!P || !T || !S || M <= 0 || N <= 0 || E <= 0 || batch <= 0 || t_rpi < 0 || lds < N || (ST && lds < M)) return CPC_EINVAL;
    if (batch > 1 && s_batch < (long long)lds * (ST ? std::max(M, N) : M)) return CPC_EINVAL;
    if (dtype != CPC_DTYPE_F32 && dtype != CPC_DTYPE_BF16) return CPC_EINVAL;
    return launch_diff_scores(P, T, S, ST, M, N, E, ldp, ldt, t_rpi, t_item, p_batch, t_batch, s_batch, batch, lds, dtype, (hipStream_t)stream);
}

int cpc_diff_scores_bwd(void* G, const float* S, float* sums, void* GT, const float* ST, float* sumsT, int M, int N, int lds,
                        long long s_batch, int batch, int dtype, void* stream) {
    if (!G || !S || !sums || M <= 0 || N <= 0 || batch <= 0 || lds < N) return CPC_EINVAL;
    if (GT && (!ST || !sumsT || lds < M)) return CPC_EINVAL;
    if (batch > 1 && s_batch < (long long)lds * (GT ? std::max(M, N) : M)) return CPC_EINVAL;
    if (dtype != CPC_DTYPE_F32 && dtype != CPC_DTYPE_BF16) return CPC_EINVAL;
    return launch_diff_scores_bwd(G, S, sums, GT, ST, sumsT, M, N, lds, s_batch, batch, dtype, (hipStream_t)stream);
}

int cpc_diff_scores_rank1(const float* mu, const void* X, void* out, int rows, int E, int rpi, long long item, long long ld, int dtype,
                          void* stream) {
    if (!mu || !X || !out || rows <= 0 || E <= 0 || rpi < 0) return CPC_EINVAL;
    if (dtype != CPC_DTYPE_F32 && dtype != CPC_DTYPE_BF16) return CPC_EINVAL;
    return launch_diff_scores_rank1(mu, X, out, rows, E, rpi, item, ld, dtype, (hipStream_t)stream);
}

// (the argument checks shared by cpc_norm_rows and cpc_norm_rows_bwd)
static bool norm_rows_args_ok(int rows, int E, int rpi, float scale, float eps, int dtype) {
    return rows >= 1 && E >= 1 && E <= 4096 && rpi >= 0 && std::isfinite(scale) && scale > 0.f && std::isfinite(eps) && eps > 0.f &&
           (dtype == CPC_DTYPE_F32 || dtype == CPC_DTYPE_BF16);
}

int cpc_norm_rows(const void* X, void* Y, float* inv, int rows, int E, int rpi, long long item, long long ld, float scale, float eps,
                  int dtype, void* stream) {
    if (!X || !Y || !inv || !norm_rows_args_ok(rows, E, rpi, scale, eps, dtype)) return CPC_EINVAL;
    return launch_norm_rows(X, Y, inv, rows, E, rpi, item, ld, scale, eps, dtype, (hipStream_t)stream);
}

int cpc_norm_rows_bwd(const void* Y, const float* inv, void* G, int rows, int E, int rpi, long long item, long long ld, float scale,
                      float eps, int dtype, void* stream) {
    if (!Y || !inv || !G || !norm_rows_args_ok(rows, E, rpi, scale, eps, dtype)) return CPC_EINVAL;
    return launch_norm_rows_bwd(Y, inv, G, rows, E, rpi, item, ld, scale, eps, dtype, (hipStream_t)stream);
}

int cpc_norm_rows_dev(const void* X, void* Y, float* inv, int rows, int E, int rpi, long long item, long long ld, const float* scale,
                      float eps, int dtype, void* stream) {
    if (!X || !Y || !inv || !scale || !norm_rows_args_ok(rows, E, rpi, 1.f, eps, dtype)) return CPC_EINVAL;
    return launch_norm_rows_dev(X, Y, inv, rows, E, rpi, item, ld, scale, eps, dtype, (hipStream_t)stream);
}

int cpc_norm_rows_bwd_dev(const void* Y, const float* inv, void* G, float* dots, int rows, int E, int rpi, long long item, long long ld,
                          const float* scale, float eps, int dtype, void* stream) {
    if (!Y || !inv || !G || !dots || !scale || !norm_rows_args_ok(rows, E, rpi, 1.f, eps, dtype)) return CPC_EINVAL;
    return launch_norm_rows_bwd_dev(Y, inv, G, dots, rows, E, rpi, item, ld, scale, eps, dtype, (hipStream_t)stream);
}

int cpc_temperature_step(float* tstate, const float* dots, int rows, float lr, float beta1, float beta2, float eps, int step,
                         const float* adam_state, float grad_scale, float s_min, float s_max, const float* skip, void* stream) {
    if (!tstate || !dots || rows < 1 || (!adam_state && step < 1)) return CPC_EINVAL;
    for (float x : {lr, beta1, beta2, eps, grad_scale, s_min, s_max})
        if (!std::isfinite(x)) return CPC_EINVAL;
    if (s_min > s_max) return CPC_EINVAL;
    return launch_temperature_step(tstate, dots, rows, lr, beta1, beta2, eps, step, adam_state, grad_scale, s_min, s_max, skip,
                                   (hipStream_t)stream);
}

int cpc_temperature_set(float* tstate, int kind, double start, double end, long long total_steps, long long step, const float* adam_state,
                        long long step_offset, void* stream) {
    if (!tstate || kind < 0 || kind > 1 || total_steps < 1 || !(std::isfinite(start) && start > 0.0) || !(std::isfinite(end) && end > 0.0))
        return CPC_EINVAL;
    if (adam_state ? step_offset < 0 : step < 0) return CPC_EINVAL;
    return launch_temperature_set(tstate, kind, start, end, total_steps, step, adam_state, step_offset, (hipStream_t)stream);
}

int cpc_adam(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps, int step,
             float grad_scale, const float* skip, void* stream) {
    return launch_adam({p, g, m, v, n, lr, beta1, beta2, eps, grad_scale, skip, nullptr, 0.f, nullptr, 0}, step, false, (hipStream_t)stream);
}

long long cpc_grad_norm_workspace_floats(long long n) { return grad_norm_workspace_floats(n); }

int cpc_grad_norm(const float* g, long long n, float grad_scale, float max_norm, float* workspace, float* state, float* nan_pair,
                  void* stream) {
    return launch_grad_norm(g, n, grad_scale, max_norm, workspace, state, nan_pair, (hipStream_t)stream);
}

int cpc_adam_clip(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps, int step,
                  float grad_scale, const float* coef, const float* skip, void* stream) {
    return launch_adam({p, g, m, v, n, lr, beta1, beta2, eps, grad_scale, skip, coef, 0.f, nullptr, 0}, step, true, (hipStream_t)stream);
}

int cpc_adamw(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps, int step,
              float grad_scale, float weight_decay, const unsigned* decay_bits, long long first_block, const float* coef,
              const float* skip, void* stream) {
    return launch_adam({p, g, m, v, n, lr, beta1, beta2, eps, grad_scale, skip, coef, weight_decay, decay_bits, first_block}, step, false,
                       (hipStream_t)stream);
}

int cpc_adamw_dev(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                  float* state, float grad_scale, float weight_decay, const unsigned* decay_bits, int kind, long long warmup_steps,
                  long long total_steps, float min_ratio, long long step_offset, const float* coef, const float* skip, void* stream) {
    return launch_adam_dev({p, g, m, v, n, lr, beta1, beta2, eps, grad_scale, skip, coef, weight_decay, decay_bits, 0}, state, true, kind,
                           warmup_steps, total_steps, min_ratio, step_offset, (hipStream_t)stream);
}

int cpc_lr_factors(int kind, long long warmup_steps, long long total_steps, float min_ratio, long long step0, int count, float* out,
                   void* stream) {
    return launch_lr_factors(kind, warmup_steps, total_steps, min_ratio, step0, count, out, (hipStream_t)stream);
}

long long cpc_lamb_workspace_floats(long long total_blocks) { return lamb_workspace_floats(total_blocks); }

int cpc_lamb(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps, int step,
             float grad_scale, float weight_decay, const unsigned* select_bits, long long first_block, const float* coef,
             const int* param_block, const int* param_block_dev, const int* block_param, int first_param, int n_params,
             int total_params, float trust_clip, float* workspace, float* trust, const float* skip, void* stream) {
    return launch_lamb({p, g, m, v, n, lr, beta1, beta2, eps, grad_scale, skip, coef, weight_decay, select_bits, first_block}, step,
                       {param_block, param_block_dev, block_param, first_param, n_params, total_params, trust_clip, workspace, trust},
                       (hipStream_t)stream);
}

int cpc_ema(const float* p, float* ema, long long n, float decay, int warmup, int step, const float* state, const float* skip,
            void* stream) {
    return launch_ema(p, ema, n, decay, warmup, step, state, skip, (hipStream_t)stream);
}

int cpc_ema_swap(float* p, float* ema, long long n, void* stream) { return launch_ema_swap(p, ema, n, (hipStream_t)stream); }

int cpc_wave_power_chunks(int n) { return wave_power_chunks(n); }

// (the shape checks shared by cpc_wave_power and cpc_wave_augment; blockIdx.y carries the clip, f32 carries sample indices)
static bool wave_shape_ok(int B, int L, long long ld) { return B >= 1 && B <= 65535 && L >= 1 && L <= (1 << 24) && ld >= L; }

int cpc_wave_power(const float* x, float* partial, int B, int L, long long ldx, int n, void* stream) {
    if (!x || !partial || !wave_shape_ok(B, L, ldx) || n < 1 || n > L) return CPC_EINVAL;
    return launch_wave_power(x, partial, B, L, ldx, n, (hipStream_t)stream);
}

int cpc_wave_augment(const float* x, float* y, const float* partial, float* params_out, int B, int L, long long ldx, long long ldy,
                     const CpcWaveAugment* cfg, void* stream) {
    if (!x || !y || !cfg || !wave_shape_ok(B, L, ldx) || ldy < L) return CPC_EINVAL;
    if (cfg->protect_from < 0 || cfg->protect_from > L) return CPC_EINVAL;
    if (cfg->q_lo < 32768 || cfg->q_lo > cfg->q_hi || cfg->q_hi > 131072) return CPC_EINVAL;
    if (cfg->drop_count < 0 || cfg->drop_count > 8 || (cfg->drop_count > 0 && cfg->drop_max_len < 1)) return CPC_EINVAL;
    if (cfg->noise_on && (!partial || !std::isfinite(cfg->snr_lo) || !std::isfinite(cfg->snr_hi) || cfg->snr_lo > cfg->snr_hi))
        return CPC_EINVAL;
    if (cfg->gain_on && (!std::isfinite(cfg->gain_lo_db) || !std::isfinite(cfg->gain_hi_db) || cfg->gain_lo_db > cfg->gain_hi_db))
        return CPC_EINVAL;
    if (cfg->polarity_threshold > (1ull << 32)) return CPC_EINVAL;
    return launch_wave_augment(x, y, partial, params_out, B, L, ldx, ldy, cfg, (hipStream_t)stream);
}

int cpc_window_gather(const void* store, int store_code, long long store_len, const long long* starts, long long n_items,
                      const long long* idx, float* out, int B, int L, long long ldo, float scale, void* stream) {
    if (!store || !starts || !idx || !out || !wave_shape_ok(B, L, ldo) || store_len < L || n_items < 1) return CPC_EINVAL;
    if ((store_code != 0 && store_code != 1) || !std::isfinite(scale)) return CPC_EINVAL;
    if (reinterpret_cast<uintptr_t>(store) % (store_code == 1 ? 2 : 4) != 0 || reinterpret_cast<uintptr_t>(out) % 4 != 0) return CPC_EINVAL;
    return launch_window_gather(store, store_code, store_len, starts, n_items, idx, out, B, L, ldo, scale, (hipStream_t)stream);
}

int cpc_resample(const void* src, int src_code, long long src_frames_total, int C, int mix, float in_scale, const float* taps, int L,
                 int M, int W, const long long* segs, const long long* tile_first, int nseg, long long ntiles, void* dst, int dst_code,
                 long long dst_total, float out_scale, void* stream) {
    if (!src || !taps || !segs || !tile_first || !dst || C < 1 || C > 8) return CPC_EINVAL;
    if ((mix != 0 && mix != 1) || (src_code != 0 && src_code != 1) || (dst_code != 0 && dst_code != 1)) return CPC_EINVAL;
    if (L < 1 || L > (1 << 20) || M < 1 || M > (1 << 20) || W < 0 || W > (1 << 20)) return CPC_EINVAL;
    if ((long long)L * (2ll * W + 1) > (1ll << 24) || resample_span_floats(L, M, W) > 16384) return CPC_EINVAL;
    if (nseg < 1 || ntiles < 1 || ntiles > (1ll << 23)) return CPC_EINVAL;
    if (src_frames_total < 1 || src_frames_total > (1ll << 40) || dst_total < 1 || dst_total > (1ll << 40)) return CPC_EINVAL;
    if (!std::isfinite(in_scale) || !std::isfinite(out_scale)) return CPC_EINVAL;
    if (reinterpret_cast<uintptr_t>(src) % (src_code == 1 ? 2 : 4) != 0 || reinterpret_cast<uintptr_t>(dst) % (dst_code == 1 ? 2 : 4) != 0)
        return CPC_EINVAL;
    if (reinterpret_cast<uintptr_t>(taps) % 4 != 0 || reinterpret_cast<uintptr_t>(segs) % 8 != 0 ||
        reinterpret_cast<uintptr_t>(tile_first) % 8 != 0)
        return CPC_EINVAL;
    return launch_resample(src, src_code, src_frames_total, C, mix, in_scale, taps, L, M, W, segs, tile_first, nseg, ntiles, dst, dst_code,
                           dst_total, out_scale, (hipStream_t)stream);
}

// (the extents every table row of the feature-extraction calls is checked against)
static bool stream_extents_ok(long long store_len, int L, int Tc, long long total_frames, int n_rec) {
    return store_len >= 1 && L >= 1 && L <= (1 << 24) && Tc >= 1 && total_frames >= 0 && n_rec >= 1;
}
static bool aligned_to(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

int cpc_stream_gather(const void* store, int store_code, long long store_len, const long long* table, float* out, int R, int L,
                      long long ldo, float scale, int Tc, long long total_frames, int n_rec, void* stream) {
    if (!store || !table || !out || R < 1 || R > 65535 || !stream_extents_ok(store_len, L, Tc, total_frames, n_rec) || ldo < L)
        return CPC_EINVAL;
    if ((store_code != 0 && store_code != 1) || !std::isfinite(scale)) return CPC_EINVAL;
    if (!aligned_to(store, store_code == 1 ? 2 : 4) || !aligned_to(out, 4) || !aligned_to(table, 8)) return CPC_EINVAL;
    const StreamExtents ext = {store_len, total_frames, L, Tc, n_rec};
    return launch_stream_gather(store, store_code, table, ext, out, R, ldo, scale, (hipStream_t)stream);
}

int cpc_feature_emit(const long long* table, const void* top, long long top_item, const void* hall, long long hall_item, int src_dtype,
                     void* z_out, void* c_out, int out_dtype, int R, int Tc, int E, int H, long long store_len, int L,
                     long long total_frames, int n_rec, double* partial, double* acc_z, double* acc_c, void* stream) {
    if (!table || (!z_out && !c_out) || (z_out && !top) || (c_out && !hall)) return CPC_EINVAL;
    if ((src_dtype != CPC_DTYPE_F32 && src_dtype != CPC_DTYPE_BF16) || (out_dtype != CPC_DTYPE_F32 && out_dtype != CPC_DTYPE_BF16))
        return CPC_EINVAL;
    if (R < 1 || R > 65535 || !stream_extents_ok(store_len, L, Tc, total_frames, n_rec) || Tc > (1 << 20)) return CPC_EINVAL;
    const int ch = src_dtype == CPC_DTYPE_BF16 ? 8 : 4;
    if (E < 0 || H < 0 || E % ch || H % ch || E > 65536 || H > 65536) return CPC_EINVAL;
    if (z_out && (E < ch || top_item < (long long)Tc * E || top_item % ch || !aligned_to(top, 16) || !aligned_to(z_out, 16)))
        return CPC_EINVAL;
    if (c_out && (H < ch || hall_item < ((long long)Tc + 1) * H || hall_item % ch || !aligned_to(hall, 16) || !aligned_to(c_out, 16)))
        return CPC_EINVAL;
    if (partial) {
        if (!aligned_to(partial, 16) || (z_out && (!acc_z || !aligned_to(acc_z, 8))) || (c_out && (!acc_c || !aligned_to(acc_c, 8))))
            return CPC_EINVAL;
    }
    if (!aligned_to(table, 8)) return CPC_EINVAL;
    const StreamExtents ext = {store_len, total_frames, L, Tc, n_rec};
    return launch_feature_emit(table, ext, top, top_item, hall, hall_item, src_dtype, z_out, c_out, out_dtype, R, E, H, partial, acc_z,
                               acc_c, (hipStream_t)stream);
}

int cpc_stream_carry(const long long* table, const float* const* src, float* const* dst, int nstate, int R, int H, long long store_len,
                     int L, int Tc, long long total_frames, int n_rec, void* stream) {
    if (!table || !src || !dst || nstate < 1 || nstate > CPC_STREAM_MAX_STATES) return CPC_EINVAL;
    if (R < 1 || R > 65535 || H < 4 || H > 65536 || H % 4 || !stream_extents_ok(store_len, L, Tc, total_frames, n_rec)) return CPC_EINVAL;
    if (!aligned_to(table, 8)) return CPC_EINVAL;
    for (int i = 0; i < nstate; ++i) {
        if (!src[i] || !dst[i] || !aligned_to(src[i], 16) || !aligned_to(dst[i], 16)) return CPC_EINVAL;
        for (int j = 0; j < nstate; ++j)
            if (dst[i] == src[j]) return CPC_EINVAL;
    }
    const StreamExtents ext = {store_len, total_frames, L, Tc, n_rec};
    return launch_stream_carry(table, ext, src, dst, nstate, R, H, (hipStream_t)stream);
}

// (the shape limits the three k-means calls share)
static bool kmeans_shape_ok(const void* x, int dtype, long long N, int D, long long ldx, int K) {
    if (!x || (dtype != CPC_DTYPE_F32 && dtype != CPC_DTYPE_BF16)) return false;
    if (N < 1 || N > 0x7FFFFFFFll || D < 16 || D > 512 || D % 16 || K < 2 || K > 1024) return false;
    const int ch = dtype == CPC_DTYPE_BF16 ? 8 : 4;
    return ldx >= D && ldx % ch == 0 && aligned_to(x, 16);
}

int cpc_kmeans_assign(const void* x, int dtype, long long N, int D, long long ldx, const float* centers, const float* cnorm, int K,
                      int* labels, float* dist, void* stream) {
    if (!kmeans_shape_ok(x, dtype, N, D, ldx, K) || !centers || !cnorm || !labels) return CPC_EINVAL;
    if (!aligned_to(centers, 16) || !aligned_to(cnorm, 4) || !aligned_to(labels, 4) || !aligned_to(dist, 4)) return CPC_EINVAL;
    return launch_kmeans_assign(x, dtype, N, D, ldx, centers, cnorm, K, labels, dist, (hipStream_t)stream);
}

long long cpc_kmeans_scratch_bytes(long long N, int K, int D) {
    if (N < 1 || N > 0x7FFFFFFFll || D < 16 || D > 512 || D % 16 || K < 2 || K > 1024) return CPC_EINVAL;
    return kmeans_scratch_bytes(N, K, D);
}

int cpc_kmeans_update(const void* x, int dtype, long long N, int D, long long ldx, const int* labels, const float* dist,
                      const float* centers_old, int K, void* scratch, long long scratch_bytes, float* centers_new, float* cnorm,
                      int* counts, double* inertia, void* stream) {
    if (!kmeans_shape_ok(x, dtype, N, D, ldx, K) || !labels || !centers_old || !scratch || !centers_new || !cnorm || !counts)
        return CPC_EINVAL;
    if ((dist == nullptr) != (inertia == nullptr)) return CPC_EINVAL;
    if (scratch_bytes < kmeans_scratch_bytes(N, K, D) || !aligned_to(scratch, 16)) return CPC_EINVAL;
    if (!aligned_to(labels, 4) || !aligned_to(dist, 4) || !aligned_to(centers_old, 4) || !aligned_to(centers_new, 4) ||
        !aligned_to(cnorm, 4) || !aligned_to(counts, 4) || !aligned_to(inertia, 8))
        return CPC_EINVAL;
    return launch_kmeans_update(x, dtype, N, D, ldx, labels, dist, centers_old, K, scratch, centers_new, cnorm, counts, inertia,
                                (hipStream_t)stream);
}

int cpc_kmeans_cnorm(const float* centers, float* cnorm, int K, int D, void* stream) {
    if (!centers || !cnorm || D < 16 || D > 512 || D % 16 || K < 2 || K > 1024) return CPC_EINVAL;
    if (!aligned_to(centers, 4) || !aligned_to(cnorm, 4)) return CPC_EINVAL;
    return launch_kmeans_cnorm(centers, cnorm, K, D, (hipStream_t)stream);
}

// (the store limits the frame-distance and DTW calls share with the k-means calls, and the metric)
static bool dtw_store_ok(const void* x, int dtype, long long N, int D, long long ldx, int metric) {
    return kmeans_shape_ok(x, dtype, N, D, ldx, 2) && metric >= 0 && metric <= 2;
}

int cpc_frame_distance(const void* x, int dtype, long long N, int D, long long ldx, long long a_first, int La, long long b_first, int Lb,
                       int metric, float* out, long long ldo, void* stream) {
    if (!dtw_store_ok(x, dtype, N, D, ldx, metric) || !out || !aligned_to(out, 4)) return CPC_EINVAL;
    if (La < 1 || La > 128 || Lb < 1 || Lb > 128 || a_first < 0 || a_first > N - La || b_first < 0 || b_first > N - Lb || ldo < Lb)
        return CPC_EINVAL;
    return launch_frame_distance(x, dtype, D, ldx, a_first, La, b_first, Lb, metric, out, ldo, (hipStream_t)stream);
}

int cpc_dtw(const void* x, int dtype, long long N, int D, long long ldx, const long long* pairs, long long P, int metric, float* dist,
            float* cost, int* path_len, void* stream) {
    if (!dtw_store_ok(x, dtype, N, D, ldx, metric) || !pairs || !dist || P < 1 || P > 0x7FFFFFFFll) return CPC_EINVAL;
    if (!aligned_to(pairs, 8) || !aligned_to(dist, 4) || !aligned_to(cost, 4) || !aligned_to(path_len, 4)) return CPC_EINVAL;
    return launch_dtw(x, dtype, N, D, ldx, pairs, P, metric, dist, cost, path_len, (hipStream_t)stream);
}

int cpc_abx_count(const float* dist, long long n_dist, const long long* tasks, long long T, long long* out, void* stream) {
    if (!dist || !tasks || !out || n_dist < 1 || T < 1 || T > 0x7FFFFFFFll) return CPC_EINVAL;
    if (!aligned_to(dist, 4) || !aligned_to(tasks, 8) || !aligned_to(out, 8)) return CPC_EINVAL;
    return launch_abx_count(dist, n_dist, tasks, T, out, (hipStream_t)stream);
}

int cpc_grid_sum_chunks(int n) { return grid_sum_chunks(n); }

int cpc_grid_sum(const float* x, float* partial, int B, int n, long long ldb, int Cc, void* stream) {
    if (!x || !partial || B < 1 || B > 65535 || (Cc != 1 && Cc != 2 && Cc != 4) || n < 1 || n % Cc != 0 || ldb < n) return CPC_EINVAL;
    return launch_grid_sum(x, partial, B, n, ldb, Cc, (hipStream_t)stream);
}

int cpc_grid_mask(const float* x, float* y, const float* partial, int* spans_out, float* fill_out, int B, int W, int H, int Cc,
                  long long ldbx, long long ldby, const CpcGridMask* cfg, void* stream) {
    if (!x || !y || !cfg || B < 1 || B > 65535 || W < 1 || H < 1 || (Cc != 1 && Cc != 2 && Cc != 4)) return CPC_EINVAL;
    const long long n = (long long)W * H * Cc;
    if (n > 0x7FFFFFFFll || ldbx < n || ldby < n) return CPC_EINVAL;
    if (cfg->protect_last < 0 || cfg->protect_last > W) return CPC_EINVAL;
    if (cfg->freq_count < 0 || cfg->freq_count > 8 || cfg->time_count < 0 || cfg->time_count > 8 || cfg->freq_max < 0) return CPC_EINVAL;
    if (cfg->time_cap < 0 || cfg->time_cap > W - cfg->protect_last) return CPC_EINVAL;
    if (cfg->fill_mode < 0 || cfg->fill_mode > 2 || (cfg->fill_mode == 1 && !std::isfinite(cfg->fill_value))) return CPC_EINVAL;
    if (cfg->fill_mode == 2 && !partial) return CPC_EINVAL;
    if (x == y) {
        if (ldbx != ldby) return CPC_EINVAL;
    } else {          // the clip ranges of two different buffers must not meet
        const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y;
        const uintptr_t xe = xa + 4 * (uintptr_t)((long long)(B - 1) * ldbx + n), ye = ya + 4 * (uintptr_t)((long long)(B - 1) * ldby + n);
        if (xa < ye && ya < xe) return CPC_EINVAL;
    }
    return launch_grid_mask(x, y, partial, spans_out, fill_out, B, W, H, Cc, ldbx, ldby, cfg, (hipStream_t)stream);
}

int cpc_mel_pointwise(const float* spec, long long lds, const int* band_lo, const int* band_n, const int* band_off, const float* band_w,
                      float* out, int B, int Tn, int n_freq, int n_mels, int delta, int take_log, float log_offset, float scaling,
                      float delta_scaling, void* stream) {
    if (!spec || !band_lo || !band_n || !band_off || !band_w || !out) return CPC_EINVAL;
    if ((delta != 0 && delta != 1) || (take_log != 0 && take_log != 1) || (delta && !take_log)) return CPC_EINVAL;
    if (B < 1 || n_mels < 1 || n_mels > 1024 || n_freq < 2 || n_freq > 4097 || Tn < 1 + delta) return CPC_EINVAL;
    if (lds < 2LL * n_freq || (lds & 1)) return CPC_EINVAL;
    if (((uintptr_t)spec & 7) || (delta && ((uintptr_t)out & 7))) return CPC_EINVAL;      // float2 loads of the rows, float2 stores with delta
    if (take_log && (!std::isfinite(log_offset) || log_offset <= 0.f)) return CPC_EINVAL;
    if (!std::isfinite(scaling) || !std::isfinite(delta_scaling)) return CPC_EINVAL;
    return launch_mel_pointwise(spec, lds, band_lo, band_n, band_off, band_w, out, B, Tn, n_freq, n_mels, delta, take_log, log_offset, scaling,
                                delta_scaling, (hipStream_t)stream);
}

}  // extern "C"
