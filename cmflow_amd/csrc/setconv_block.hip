// Host-side orchestration of one set-conv block (PointLocalFeature, utils/model_utils/radarflow_util.py:144-162)
// forward and backward as ONE C-ABI call each.
//
// The block is ~25 kernel launches forward and ~45 backward, most of them a few microseconds long at N = 256.
// Issued one by one from Python (ctypes call + tensor allocations + autograd bookkeeping, ~10-15 us each)
// the first encoder of the model was entirely host bound (1.3 ms per call for ~0.2 ms of GPU work).  Here the
// whole sequence is enqueued from C++ into caller-provided arenas; the kernels and their order are exactly
// those of cmflow_amd/fused_blocks.py's SetConvFn (and MLPChainFn for cmf_mlp_forward / _backward at the end of the
// file), which remain the readable specification.  The product calls arrive from the same module: SetConvBlockFn (one
// block), MultiScaleBlockFn / DualCloudBlockFn (the blocks of an encoder call: queries, heads / bodies on the stream
// pool or batched, batched tails) and MLPChainBlockFn, with descriptors filled by _fill_setconv_desc / _fill_bn.
//
// In code a layer is the index l of the BatchNorm it ends in, as in the descriptor's arrays: l = 0 the hoisted first conv,
// 1 .. 2 per neighbour slot (M = B N S rows), the max over the ball, 3 .. 5 per point (P = B N rows); conv layer l (1 .. 5)
// has weights d->w[l - 1].  The prose counts from one as the reference does ("layers 4-6" = l = 3 .. 5).
#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>
#include "cmf_common.h"
#include "gemm_args.h"
#include "../../include/cmflow_hip.h"

namespace {

#define CMF_TRY(call) do { int e_ = (call); if (e_) return e_; } while (0)

// the A/B switches of this file (each on unless its variable starts with '0')
inline bool thin_fused_on() { static const bool on = cmf_env_on("CMF_THIN_FUSED"); return on; }
inline bool thin_wide_on() { static const bool on = cmf_env_on("CMF_THIN_WIDE"); return on; }
inline bool body_batch_on() { static const bool on = cmf_env_on("CMF_BODY_BATCH"); return on; }
inline bool tail_batch_on() { static const bool on = cmf_env_on("CMF_TAIL_BATCH"); return on; }
inline bool train_gather_on() { static const bool on = cmf_env_on("CMF_TRAIN_GATHER"); return on; }
inline bool train_gather_sum_on() { static const bool on = cmf_env_on("CMF_TRAIN_GATHER_SUM"); return on; }
inline bool bnb_gather_on() { static const bool on = cmf_env_on("CMF_BNB_GATHER"); return on; }

// training through the register chain (csrc/setconv_chain.hip): the narrow block's slot-level activations z1 / z2 / z3 are never stored
// -- every pass recomputes them from the gathered per-point rows; z3's slot of `saved` holds the selected pre-activations (P x C3).
// Eval-mode BatchNorm with a backward pass to follow only (the regime of every epoch after the first in the reference's loop: no
// statistics passes): three passes against seven per-layer kernels -- 1.25 against 1.50 ms.  [With train-mode BN (round 5, removed)
// the two statistics passes made it five chain passes at 1.64 ms against 1.50 ms for the per-layer kernels: at 64 K .. 512 K rows
// per launch the passes' fixed costs (constants and weights into LDS per workgroup, a statistics row per wave, the re-gather per
// pass) ate what the 3x lower HBM traffic saved.]  Inference (one pass, cmf_setconv_chain_infer) is where the chain pays most:
// forward 5.91 -> 5.56 ms.
// Which way a block's neighbour-slot layers go -- 0: the per-layer kernels, 1: the chain's inference pass (no backward call to follow),
// 2: the chain's training passes (a backward call follows; its statistics rows want whole 128-row tiles).  The ONE predicate behind
// the dispatch of cmf_setconv_forward / _backward, the batched inference launch and cmf_setconv_path.
inline int setconv_path(const cmf_setconv_desc *d)
{
    const long long M = (long long)d->B * d->N * d->S;
    if (d->training || !cmf_setconv_chain_supported(d->N, d->S, d->O1, d->C[0], d->C[1], M) || d->ldy % 4 != 0 || ((uintptr_t)d->y & 15) != 0)
        return 0;
    if (d->inference) return 1;
    return M % 128 == 0 ? 2 : 0;
}
inline bool chain_train(const cmf_setconv_desc *d) { return setconv_path(d) == 2; }

struct Bump {
    float *base;
    size_t off;
    explicit Bump(float *b) : base(b), off(0) {}
    float *take(size_t n)
    {
        float *p = base ? base + off : nullptr;
        off += (n + 63) / 64 * 64;                       // 256-byte granules: every buffer 16-byte aligned
        return p;
    }
};

inline int dw_split(long long M, int N, int K);
// the gathering weight gradient's split: the count its 256-row tiles go with, else the usual choice
inline int dwg_split(long long M, int N, int K)
{
    const int s = cmf_gemm_dw_gather_split(N, K, M);
    return s ? s : dw_split(M, N, K);
}

inline int tiles128(long long rows) { return (int)((rows + 127) / 128); }

// split-K choice of fused_blocks.gemm_dw (positions M contracted into an N x K weight gradient)
inline int dw_split(long long M, int N, int K)
{
    if (N <= 64 && K <= 64) return (int)std::max<long long>(2, std::min<long long>(M / 128, 1024));   // thin kernel: slab per workgroup, >= 128 rows each
    // tiled kernel: slabs are dealt to the 8 XCDs (split % 8), so the split is a multiple of 8; among the candidates
    // take the one with the smallest wave-quantised cost: waves of 768 resident workgroups x (chunks per workgroup +
    // a fixed per-workgroup overhead of ~12 chunks).  [A "fill 512 workgroups" rule gave the 2048 x 1028 gradient of the
    // stacked first conv a split of 4: half the XCDs idle, 1.55 ms instead of 0.73 ms.]
    const long long tiles = (long long)((N + 127) / 128) * ((K + 127) / 128);
    const long long chunks = (M + 15) / 16;
    if (chunks < 64) return 1;
    static const int cand[] = {8, 16, 24, 32, 48, 64, 96, 128, 256, 384};     // 256 / 384: one- and two-tile outputs (64 x 256 over 524288 rows: 242 -> 203 us)
    int best = 8;
    double best_cost = 1e30;
    for (int s : cand) {
        if (chunks / s < 8) break;
        const double cost = (double)((tiles * s + 767) / 768) * ((double)chunks / s + 12.0);
        if (cost < best_cost) { best_cost = cost; best = s; }
    }
    return best;
}

// One layer's folded BatchNorm block in `saved`: mean | invstd | a | c (4 * C floats; y = relu(a z + c)).  The only host code
// that spells the order out.  All null: no BatchNorm in front (an input that is already active).
struct Bn {
    float *mean, *invstd, *a, *c;
    Bn() : mean(nullptr), invstd(nullptr), a(nullptr), c(nullptr) {}
    Bn(float *block, int C) : mean(block), invstd(block ? block + C : nullptr), a(block ? block + 2 * C : nullptr), c(block ? block + 3 * C : nullptr) {}
    float *block() const { return mean; }         // the whole block (the fold kernels and the register chain address it themselves)
};

struct Layout {
    // saved for backward
    int *idx, *offsets, *inv;
    float *dxyz, *z1, *z2, *z3, *x, *z4, *z5, *z6, *fwd_sums;
    unsigned char *argmax;
    float *zsel;                  // (P, C3) pre-activations of layer 3 at the arg-max slots (per-layer path; the chain keeps them in z3's slot)
    Bn bn[6];
    // scratch
    float *partial, *partial_x, *sums, *t6, *t5, *t4, *dx, *dU3, *dU2, *dU1, *splitk;
    float *dZ2;                   // dZ of BN layer 1, written by the gathering weight-gradient GEMM that fuses its BN backward (or null)
    size_t saved_floats, scratch_floats;
    // per layer l = 0 .. 5: the pre-activations of BN layer l and the gradient with respect to them; per conv layer l = 1 .. 5: its
    // input, the BatchNorm in front of it and the gradient into that input (l = 3 reads the pooled rows x, already active)
    float *z(int l) const { float *const v[6] = {z1, z2, z3, z4, z5, z6}; return v[l]; }
    float *dU(int l) const { float *const v[6] = {dU1, dU2, dU3, t4, t5, t6}; return v[l]; }
    float *zin(int l) const { return l == 3 ? x : z(l - 1); }
    float *dUin(int l) const { return l == 3 ? dx : dU(l - 1); }
    Bn bn_in(int l) const { return l == 3 ? Bn() : bn[l - 1]; }
};

inline int chan(const cmf_setconv_desc *d, int layer)       // out channels of BN layer 0..5
{
    return layer == 0 ? d->O1 : d->C[layer - 1];
}
inline long long rows_of(const cmf_setconv_desc *d, int layer)      // rows of BN layer 0..5: neighbour slots, behind the max points
{
    return (long long)d->B * d->N * (layer <= 2 ? d->S : 1);
}

// The arenas are sized by PATH (VERDICT r5 item 7 / ADVICE r4).  A block that never materialises its grouped first-layer tensor
// (gather_layout: the second encoder's shapes) keeps in that tensor's slot of `saved` only what the gathering GEMMs read -- M row
// indices and the three coordinate planes of Wx -- instead of M x O1 floats (1 GB at the largest scale, B = 64); and the slot of
// the data gradient into that layer in the backward scratch holds, when the gradient is summed inside the GEMM
// (gather_sum_shape and an input gradient wanted: make_layout's sum_in_gemm), the pieces matrix, the permutation, the permuted
// source points and relative coordinates.  Both predicates are pure functions of the descriptor's SHAPE fields:
// cmf_setconv_sizes, the forward and the backward call must agree on them, so the pointer-alignment
// conditions of the gathering kernels are NOT part of them -- a block with the compact layout and a misaligned y is refused
// (CMF_CHECK_ARG in the calls) instead of overrunning a slot that was never sized for the materialised tensor.  Whether a
// backward call wants the input gradient (d->dy set) is the CALL's business: the backward entry points pass it to make_layout,
// cmf_setconv_sizes reports the scratch size of either case and reads no output pointer.
// CMF_TRAIN_GATHER=0 / CMF_TRAIN_GATHER_SUM=0 (A/B) bring the materialised sizes back.
//
// gather_layout -- training without the grouped first-layer tensor (second-encoder shapes, train-mode or eval-mode BatchNorm alike): the
// forward pass takes the layer's statistics from cmf_group_affine's statistics-only form and the three GEMMs that read the tensor form
// it from the per-point rows (cmf_gemm_gather_affine / cmf_gemm_dx_gather / cmf_gemm_dw_gather: each bit-identical to its materialised
// counterpart).  The slot is sized for the gathering form, so there is no other form to fall back to.
// gather_sum_layout -- ... and, when the input gradient is wanted, without the data gradient into the first layer either (M x O1 again):
// the GEMM walks the slots in inverse-index order and reduces runs of equal source points in its epilogue (cmf_gemm_dx_gather_sum); the
// scatter at the end of the block adds a point's pieces.
inline bool gather_layout(const cmf_setconv_desc *d)
{
    const long long M = (long long)d->B * d->N * d->S;
    return train_gather_on() && M % 128 == 0 && M < (1ll << 31) && d->C[0] % 128 == 0 && d->O1 % 128 == 0 && d->ldy % 4 == 0;
}
inline bool gather_sum_shape(const cmf_setconv_desc *d) { return train_gather_sum_on() && gather_layout(d) && d->S >= 2; }
inline bool gather_sum_layout(const cmf_setconv_desc *d) { return gather_sum_shape(d) && d->dy != nullptr; }   // of a backward call

// BN backward of the layer behind the gathered first layer inside its weight-gradient GEMM (cmf_gemm_dw_gather_bn_bwd): the stand-alone
// pass over (M, C2) -- read dU, read Z, write dZ: 3 GB per step at B = 64 -- goes, dZ lands in a buffer of its own for the data-gradient
// GEMM (other column tiles of the slab still read dU).  Bit-identical to the two-kernel form.  [measured, round 6, A/B/A/B on one box:
// 18.999 / 19.035 -> 18.809 / 18.844 ms per step; the four GEMMs that absorb the pass run 2 points further from their MFMA roof --
// isolated cmf_gemm 0.739 -> 0.719 -- which is what the round-3 form of this fusion (non-gathering, 0.1 ms per step: since removed) was
// left opt-in for: the step is the figure of merit.]  CMF_BNB_GATHER=0: the stand-alone pass (A/B).
inline bool bnb_gather(const cmf_setconv_desc *d)
{
    return bnb_gather_on() && d->training && gather_layout(d) && ((long long)d->B * d->N * d->S) >= 32768;
}

// sum_in_gemm (backward only): the call produces the input gradient, so a gather_sum_shape block sums the first layer's data gradient
// inside the GEMM and its dU1 slot is the compact one
Layout make_layout(const cmf_setconv_desc *d, float *saved, float *scratch, bool backward, bool sum_in_gemm = false)
{
    Layout L;
    const long long P = (long long)d->B * d->N, M = P * d->S;
    const int O1 = d->O1, C2 = d->C[0], C3 = d->C[1], C4 = d->C[2], C5 = d->C[3], C6 = d->C[4];
    Bump s(saved);
    L.idx = (int *)s.take(M);
    L.offsets = (int *)s.take((size_t)d->B * (d->N + 1));
    L.inv = (int *)s.take(M);
    L.dxyz = s.take(M * 4);
    L.z1 = s.take(gather_layout(d) ? (size_t)((M + 3) / 4 * 4) + 3 * (size_t)O1 : (size_t)M * O1);
    L.z2 = s.take(M * C2);
    L.z3 = s.take(M * C3);
    L.argmax = (unsigned char *)s.take((P * C3 + 3) / 4);
    L.x = s.take(P * C3);
    L.z4 = s.take(P * C4);
    L.z5 = s.take(P * C5);
    L.z6 = s.take(P * C6);
    L.fwd_sums = s.take(3 * O1 + 4);
    for (int l = 0; l < 6; ++l) L.bn[l] = Bn(s.take(4 * (size_t)chan(d, l)), chan(d, l));
    L.zsel = s.take(P * C3);       // (behind everything else: the offsets of the older slots are part of the Python side's contract)
    L.saved_floats = s.off;

    Bump t(scratch);
    const int cmax = std::max({O1, C2, C3, C4, C5, C6});
    L.partial = t.take((size_t)tiles128(M) * 5 * cmax);
    L.partial_x = t.take((size_t)tiles128(M) * (3 * O1 + 4));
    L.sums = t.take(5 * (size_t)cmax);
    if (backward) {
        L.t6 = t.take(P * C6);
        L.t5 = t.take(P * C5);
        L.t4 = t.take(P * C4);
        L.dx = t.take(P * C3);
        L.dU3 = t.take(M * C3);
        L.dU2 = t.take(M * C2);
        // (summed inside the GEMM: pieces (P + M/64) x O1 | perm M | source points M | relative coordinates 4 M -- sum_slots below)
        L.dU1 = t.take(sum_in_gemm && gather_sum_shape(d) ? (size_t)(P + M / 64) * O1 + 6 * (size_t)M : (size_t)M * O1);
        L.dZ2 = bnb_gather(d) ? t.take(M * C2) : nullptr;
        size_t sk = 0;
        sk = std::max(sk, (size_t)dw_split(P, C6, C5) * C6 * C5);
        sk = std::max(sk, (size_t)dw_split(P, C5, C4) * C5 * C4);
        sk = std::max(sk, (size_t)dw_split(P, C4, C3) * C4 * C3);
        sk = std::max(sk, (size_t)dw_split(M, C3, C2) * C3 * C2);
        sk = std::max(sk, (size_t)dw_split(M, C2, O1) * C2 * O1);
        sk = std::max(sk, (size_t)dwg_split(M, C2, O1) * C2 * O1);
        // the fused single-pass layers write their own slab counts (one slab per workgroup): size for those as well --
        // the wide form's tiles128(M) slabs of 64 x C2 exceed the dw_split-based sizes for 128 <= M < 1024 rows
        const struct { long long rows; int cout, cin; } lay[5] = {{P, C6, C5}, {P, C5, C4}, {P, C4, C3}, {M, C3, C2}, {M, C2, O1}};
        for (const auto &l : lay)
            if (cmf_thin_bwd_supported(l.cout, l.cin)) sk = std::max(sk, (size_t)cmf_thin_bwd_slabs(l.rows, nullptr) * l.cout * l.cin);
        if (cmf_thin_bwd_wide_supported(C3, C2)) sk = std::max(sk, (size_t)cmf_thin_bwd_wide_slabs(M, C2, nullptr) * 64 * C2);
        if (cmf_setconv_chain_supported(d->N, d->S, O1, C2, C3, M)) sk = std::max(sk, (size_t)(cmf_setconv_chain_waves(M, 1) / 4) * C3 * C2);
        L.splitk = t.take(sk);
    } else {
        L.t6 = L.t5 = L.t4 = L.dx = L.dU3 = L.dU2 = L.dU1 = L.splitk = L.dZ2 = nullptr;
    }
    L.scratch_floats = t.off;
    return L;
}

// Eval mode: the six folds depend on nothing the block computes (running statistics), so they are ONE launch at the head
// of the chain instead of six tiny kernels between its GEMMs.  Same arithmetic as bn_finalize_kernel's eval branch.
struct FoldAll { int C[6]; const float *gamma[6], *beta[6], *rmean[6], *rvar[6]; float eps[6]; float *out[6]; };

__global__ __launch_bounds__(256) void bn_fold_eval_kernel(const FoldAll f)
{
    const int l = blockIdx.x, C = f.C[l];
    float *b = f.out[l];
    for (int ch = threadIdx.x; ch < C; ch += 256) {
        const double mean = f.rmean[l][ch], var = f.rvar[l][ch];
        const double invstd = 1.0 / sqrt(var + (double)f.eps[l]);
        const double a = (f.gamma[l] ? (double)f.gamma[l][ch] : 1.0) * invstd;
        b[ch] = (float)mean; b[C + ch] = (float)invstd; b[2 * C + ch] = (float)a;
        b[3 * C + ch] = (float)((f.beta[l] ? (double)f.beta[l][ch] : 0.0) - mean * a);
    }
}

__global__ __launch_bounds__(256) void bn_fold_eval_batch_kernel(const CmfBatch<FoldAll> b)
{
    const FoldAll &f = b.a[blockIdx.y];
    const int l = blockIdx.x, C = f.C[l];
    float *o = f.out[l];
    for (int ch = threadIdx.x; ch < C; ch += 256) {
        const double mean = f.rmean[l][ch], var = f.rvar[l][ch];
        const double invstd = 1.0 / sqrt(var + (double)f.eps[l]);
        const double a = (f.gamma[l] ? (double)f.gamma[l][ch] : 1.0) * invstd;
        o[ch] = (float)mean; o[C + ch] = (float)invstd; o[2 * C + ch] = (float)a;
        o[3 * C + ch] = (float)((f.beta[l] ? (double)f.beta[l][ch] : 0.0) - mean * a);
    }
}

FoldAll fold_all_args(const cmf_setconv_desc *d, const Layout &L)
{
    FoldAll f;
    for (int l = 0; l < 6; ++l) {
        f.C[l] = chan(d, l); f.gamma[l] = d->gamma[l]; f.beta[l] = d->beta[l]; f.rmean[l] = d->rmean[l]; f.rvar[l] = d->rvar[l];
        f.eps[l] = d->eps[l]; f.out[l] = L.bn[l].block();
    }
    return f;
}

int fold_all_eval(const cmf_setconv_desc *d, const Layout &L, void *st)
{
    for (int l = 0; l < 6; ++l) CMF_CHECK_ARG(d->rmean[l] && d->rvar[l]);
    hipLaunchKernelGGL(bn_fold_eval_kernel, dim3(6), dim3(256), 0, (hipStream_t)st, fold_all_args(d, L));
    return cmf_launch_status();
}

// ---- one builder per argument block ----------------------------------------------------------------------------------
// The batched loops collect the structs; a single launch hands the same struct's fields to the positional entry point (never to
// a _batch entry point with n = 1: that is another kernel).  D: cmf_setconv_desc or cmf_mlp_desc.

// BN fold of layer l from `rows` rows' statistics in `partial` (train mode: batch statistics + running-statistics update)
template <class D> CmfBnFinArgs bn_fin_args(const D *d, int l, long long rows, int C, const float *partial, const Bn &b)
{
    return CmfBnFinArgs{tiles128(rows), C, (double)rows, partial, d->gamma[l], d->beta[l], d->eps[l], d->momentum[l], d->rmean[l], d->rvar[l],
                        b.mean, b.invstd, b.a, b.c, d->nbt[l]};
}
int bn_finalize(const CmfBnFinArgs &f, void *st)
{
    return cmf_bn_finalize(f.tiles, f.C, f.count, f.partial, f.gamma, f.beta, f.eps, f.momentum, f.rmean, f.rvar, f.mean_out, f.invstd_out,
                           f.a_out, f.c_out, f.nbt, st);
}
CmfBnFinArgs fold_args(const cmf_setconv_desc *d, const Layout &L, int l) { return bn_fin_args(d, l, rows_of(d, l), chan(d, l), L.partial, L.bn[l]); }
// (eval mode: the folds were done up front by fold_all_eval -- which is what makes the three exits of the forward one sequence)
int fold(const cmf_setconv_desc *d, const Layout &L, int l, void *st) { return d->training ? bn_finalize(fold_args(d, L, l), st) : 0; }

// dgamma / dbeta of BN layer l: the column sums of `tiles` rows of BN-backward partials (ncols = 2 C; the first layer's 5 C with the
// dW_xyz sums behind them), accumulated into the gradient buffers or stored there
template <class D> CmfColsumArgs bn_grad_args(const D *d, int l, int tiles, int ncols, int C, const float *partial, float *sums)
{
    return CmfColsumArgs{tiles, ncols, partial, sums, C, d->dbeta[l], d->dgamma[l], d->acc_bn[l] ? 0 : 1};
}
int bn_grad_sums(const CmfColsumArgs &c, void *st)
{
    if (c.store) return cmf_colsum_store(c.tiles, c.ncols, c.partial, c.out, c.C, c.acc0, c.acc1, st);
    return cmf_colsum(c.tiles, c.ncols, c.partial, c.out, c.C, c.acc0, c.acc1, st);
}
CmfColsumArgs bn_grad_args(const cmf_setconv_desc *d, const Layout &L, int l, int tiles)
{
    return bn_grad_args(d, l, tiles, (l == 0 ? 5 : 2) * chan(d, l), chan(d, l), L.partial, L.sums);
}

// y = relu(a z + c) behind the last layer, and its backward dU = dY * mask with the BN-backward partials
CmfAffineArgs affine_args(long long rows, int C, const float *z, const Bn &b, float *out, long long ldo)
{
    return CmfAffineArgs{rows, C, z, C, b.a, b.c, out, ldo};
}
int affine_relu(const CmfAffineArgs &a, void *st) { return cmf_affine_relu(a.M, a.C, a.z, a.ldz, a.a, a.c, a.out, a.ldo, st); }
CmfAffineArgs out_args(const cmf_setconv_desc *d, const Layout &L) { return affine_args(rows_of(d, 5), chan(d, 5), L.z6, L.bn[5], d->out, d->ldo); }

CmfActBwdArgs act_bwd_args(long long rows, int C, const float *dY, long long ldy, const float *z, const Bn &b, float *dU, float *partial)
{
    return CmfActBwdArgs{rows, C, dY, ldy, z, C, b.a, b.c, b.mean, b.invstd, dU, partial};
}
int act_bwd(const CmfActBwdArgs &a, void *st)
{
    return cmf_act_bwd_stats(a.rows, a.C, a.dY, a.ldy, a.z, a.ldz, a.a, a.c, a.mean, a.invstd, a.dU, a.partial, st);
}
CmfActBwdArgs dout_args(const cmf_setconv_desc *d, const Layout &L)
{
    return act_bwd_args(rows_of(d, 5), chan(d, 5), d->dout, d->lddout, L.z6, L.bn[5], L.t6, L.partial);
}

// ---- the three GEMMs of a layer: the only cmf_gemm calls of this file -------------------------------------------------
// Z_out = act_in(Z_in) @ W^T (+ statistics of Z_out into `stats`), Z_in (row pitch ldin) activated by the BatchNorm `in` in front
GemmArgs fwd_gemm_args(long long rows, int cin, int cout, const float *zin, long long ldin, const Bn &in, const float *w, float *zout,
                       float *stats)
{
    GemmArgs q{};
    q.M = (int)rows; q.N = cout; q.K = cin; q.A = zin; q.lda = ldin; q.B = w; q.ldb = cin; q.C = zout; q.ldc = cout;
    q.pro_a = in.a; q.pro_c = in.c; q.stats = stats; q.split_k = 1;
    return q;
}
int fwd_gemm(const GemmArgs &q, void *st)
{
    return cmf_gemm(q.M, q.N, q.K, 0, 1, q.A, q.lda, q.B, q.ldb, q.C, q.ldc, q.pro_a, q.pro_c, nullptr, nullptr, nullptr, 0, q.stats, 0,
                    nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, q.split_k, nullptr, 0, st);
}
// conv layer l = 1 .. 5 of a block
GemmArgs fwd_layer(const cmf_setconv_desc *d, const Layout &L, int l)
{
    const int cin = chan(d, l - 1);
    return fwd_gemm_args(rows_of(d, l), cin, chan(d, l), L.zin(l), cin, L.bn_in(l), d->w[l - 1], L.z(l), d->training ? L.partial : nullptr);
}

// dW[cout, cin] (+)= dZ^T @ act_in(X), X with row pitch ldx; deterministic split-K through `splitk`
int dw_gemm(long long rows, int cout, int cin, const float *dZ, const float *x, long long ldx, const Bn &in, float *dw, int accumulate,
            float *splitk, void *st)
{
    if (!dw) return 0;
    const int split = dw_split(rows, cout, cin);
    return cmf_gemm(cout, cin, (int)rows, 1, 0, dZ, cout, x, ldx, dw, cin, nullptr, nullptr, in.a, in.c, nullptr, 0, nullptr, 0,
                    nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, split, split > 1 ? splitk : nullptr, accumulate, st);
}
// dU_x (row pitch lddu) = dZ @ W, masked by the BN + ReLU `in` of x with the BN-backward partials into `stats` (and the dxyz sums when
// dxyz is given); no BatchNorm in front of x: the plain product
int dx_gemm(long long rows, int cout, int cin, const float *dZ, const float *w, float *dU, long long lddu, const float *x, const Bn &in,
            float *stats, const float *dxyz, void *st)
{
    const bool mask = in.a != nullptr;
    return cmf_gemm((int)rows, cin, cout, 0, 0, dZ, cout, w, cin, dU, lddu, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                    mask ? stats : nullptr, mask ? 1 : 0, mask ? x : nullptr, mask ? cin : 0, in.a, in.c, in.mean, in.invstd,
                    mask ? dxyz : nullptr, 1, nullptr, 0, st);
}

// the backward of conv layer l = 1 .. 5 behind BN layer l as the fused single-pass kernel's argument block (nslab: the batch call's)
CmfThinBwdCall bwd_layer_args(const cmf_setconv_desc *d, const Layout &L, int l)
{
    const int cout = chan(d, l), cin = chan(d, l - 1);
    const Bn b = L.bn[l], in = L.bn_in(l);
    CmfThinBwdCall q{};
    q.rows = rows_of(d, l); q.cout = cout; q.cin = cin; q.dU = L.dU(l); q.lddu = cout; q.z = L.z(l); q.ldz = cout;
    q.a = b.a; q.mean = b.mean; q.invstd = b.invstd; q.sums = d->training ? L.sums : nullptr;
    q.w = d->w[l - 1]; q.ldw = cin; q.x = L.zin(l); q.ldx = cin; q.in_mode = l != 3 ? 1 : 0;
    q.a_in = in.a; q.c_in = in.c; q.mean_in = in.mean; q.invstd_in = in.invstd; q.dxyz = l == 1 ? L.dxyz : nullptr;
    q.dx = L.dUin(l); q.lddx = cin; q.stats = l != 3 ? L.partial : nullptr;
    q.dw = d->dw[l - 1]; q.lddw = cin; q.accumulate = d->acc_w[l - 1]; q.slabs = L.splitk;
    return q;
}
// the slab sum behind a batched launch of such layers
CmfSplitkArgs splitk_args(const CmfThinBwdCall &q) { return CmfSplitkArgs{q.cout, q.cin, q.nslab, q.slabs, q.dw, q.lddw, q.accumulate}; }

// One backward layer: the BN-backward sums of layer l (dgamma / dbeta), then dZ -> dW (+ dU of the layer below).
// Narrow layers run the fused single-pass kernel (cmf_thin_bwd_layer: dZ is never stored); the wide ones of the second
// encoder the BN backward in place followed by the two tiled GEMMs.  CMF_THIN_FUSED=0 forces the three-kernel form.
int bwd_layer(const cmf_setconv_desc *d, const Layout &L, int l, void *st)
{
    const CmfThinBwdCall q = bwd_layer_args(d, L, l);
    CMF_TRY(bn_grad_sums(bn_grad_args(d, L, l, tiles128(q.rows)), st));
    if (thin_fused_on() && cmf_thin_bwd_supported(q.cout, q.cin))
        return cmf_thin_bwd_layer(q.rows, q.cout, q.cin, q.dU, q.lddu, q.z, q.ldz, q.a, q.mean, q.invstd, q.sums, q.w, q.ldw, q.x, q.ldx,
                                  q.in_mode, q.a_in, q.c_in, q.mean_in, q.invstd_in, q.dxyz, q.dx, q.lddx, q.stats, q.dw, q.lddw, q.accumulate,
                                  q.slabs, st);
    float *dZ = L.dU(l);                                            // in place
    CMF_TRY(cmf_bn_bwd_apply(q.rows, q.cout, dZ, q.z, q.ldz, q.a, q.mean, q.invstd, q.sums, st));
    CMF_TRY(dw_gemm(q.rows, q.cout, q.cin, dZ, q.x, q.ldx, L.bn_in(l), q.dw, q.accumulate, q.slabs, st));
    return dx_gemm(q.rows, q.cout, q.cin, dZ, q.w, q.dx, q.lddx, q.x, L.bn_in(l), q.stats, q.dxyz, st);
}

// the per-point tail of a block, forward (l = 3 .. 5 and the output activation) and backward (down to Layout::dx)
int forward_tail(const cmf_setconv_desc *d, const Layout &L, void *st)
{
    for (int l = 3; l < 6; ++l) {
        CMF_TRY(fwd_gemm(fwd_layer(d, L, l), st));
        CMF_TRY(fold(d, L, l, st));
    }
    return affine_relu(out_args(d, L), st);
}
int backward_tail(const cmf_setconv_desc *d, const Layout &L, void *st)
{
    CMF_TRY(act_bwd(dout_args(d, L), st));
    for (int l = 5; l >= 3; --l) CMF_TRY(bwd_layer(d, L, l, st));
    return 0;
}

// the head of the backward's pooled-gradient branches: the gradient of the max over the ball kept per POINT (g = L.dU3) with the
// BN-backward partials of l = 2 from the pre-activations at the arg-max slots (zsel), then that layer's dgamma / dbeta
int pooled_grad_head(const cmf_setconv_desc *d, const Layout &L, const float *zsel, void *st)
{
    const Bn &b = L.bn[2];
    const long long P = rows_of(d, 3);
    const int C3 = chan(d, 2);
    CMF_TRY(cmf_maxpool_bwd_point_sel(P, C3, L.dx, C3, zsel, b.a, b.c, b.mean, b.invstd, L.dU3, L.partial, st));
    return bn_grad_sums(bn_grad_args(d, L, 2, tiles128(P)), st);
}

// the gathering kernels' 16-byte loads: with the compact layout a misaligned operand is an argument error, not a fallback
bool gather_operands_aligned(const cmf_setconv_desc *d) { return (((uintptr_t)d->y | (uintptr_t)d->w[0]) & 15) == 0; }
int *gather_rows(const Layout &L) { return reinterpret_cast<int *>(L.z1); }
float *gather_wx3(const Layout &L, long long M) { return L.z1 + (M + 3) / 4 * 4; }

// gather_sum_layout: the slot of dU1 holds the pieces, the permutation, the permuted source points and relative coordinates
struct SumSlots { float *pieces; int *perm, *pts; float *dq2; };
SumSlots sum_slots(const cmf_setconv_desc *d, const Layout &L)
{
    const long long P = (long long)d->B * d->N, M = P * d->S;
    SumSlots s;
    s.pieces = L.dU1;
    s.perm = reinterpret_cast<int *>(L.dU1 + (P + M / 64) * d->O1);
    s.pts = s.perm + M;
    s.dq2 = reinterpret_cast<float *>(s.pts + M);
    return s;
}

// bwd_layer for the layer behind the gathered first layer: BN-backward sums, BN backward in place, weight gradient and masked data
// gradient with the first layer formed in their operand / epilogue paths
int bwd_layer1_gather(const cmf_setconv_desc *d, const Layout &L, void *st)
{
    const long long M = rows_of(d, 1);
    const int O1 = d->O1, C2 = d->C[0];
    const Bn &b = L.bn[1], &b0 = L.bn[0];
    const int *rows = gather_rows(L);
    const float *wx3 = gather_wx3(L, M);
    const int split = dwg_split(M, C2, O1);
    float *const slabs = split > 1 ? L.splitk : nullptr;
    CMF_TRY(bn_grad_sums(bn_grad_args(d, L, 1, tiles128(M)), st));
    const float *dZ2 = L.dU2;
    if (bnb_gather(d) && L.dZ2 && d->dw[0]) {
        CMF_TRY(cmf_gemm_dw_gather_bn_bwd(C2, O1, M, L.dU2, C2, L.z2, C2, b.a, b.mean, b.invstd, L.sums, L.dZ2, C2, d->y, d->ldy, rows, L.dxyz, wx3,
                                          b0.a, b0.c, d->dw[0], O1, split, slabs, d->acc_w[0], st));
        dZ2 = L.dZ2;
    } else {
        CMF_TRY(cmf_bn_bwd_apply(M, C2, L.dU2, L.z2, C2, b.a, b.mean, b.invstd, d->training ? L.sums : nullptr, st));
        if (d->dw[0])
            CMF_TRY(cmf_gemm_dw_gather(C2, O1, M, L.dU2, C2, d->y, d->ldy, rows, L.dxyz, wx3, b0.a, b0.c, d->dw[0], O1, split, slabs, d->acc_w[0], st));
    }
    if (gather_sum_layout(d)) {
        const SumSlots q = sum_slots(d, L);
        CMF_TRY(cmf_group_perm(d->B, d->N * d->S, L.inv, rows, L.dxyz, q.perm, q.pts, q.dq2, st));
        cmf_gemm_dx_gather_sum_hint((long long)d->B * d->N);
        return cmf_gemm_dx_gather_sum((int)M, O1, C2, dZ2, C2, d->w[0], O1, d->y, d->ldy, q.perm, q.pts, q.dq2, wx3, b0.a, b0.c, b0.mean, b0.invstd,
                                      q.pieces, L.partial, st);
    }
    return cmf_gemm_dx_gather((int)M, O1, C2, dZ2, C2, d->w[0], O1, L.dU1, O1, d->y, d->ldy, rows, L.dxyz, wx3, b0.a, b0.c, b0.mean, b0.invstd,
                              L.partial, st);
}

}  // namespace

extern "C" int cmf_setconv_sizes(const cmf_setconv_desc *d, long long *saved_floats, long long *scratch_fwd, long long *scratch_bwd,
                                 long long *scratch_bwd_input_grad)
{
    CMF_CHECK_ARG(d && d->B > 0 && d->N > 0 && d->S > 0 && d->S <= 64 && d->O1 % 4 == 0);
    for (int i = 0; i < 5; ++i) CMF_CHECK_ARG(d->C[i] > 0 && d->C[i] % 4 == 0);
    const Layout f = make_layout(d, nullptr, nullptr, false);
    if (saved_floats) *saved_floats = (long long)f.saved_floats;
    if (scratch_fwd) *scratch_fwd = (long long)f.scratch_floats;
    if (scratch_bwd) *scratch_bwd = (long long)make_layout(d, nullptr, nullptr, true, false).scratch_floats;
    if (scratch_bwd_input_grad) *scratch_bwd_input_grad = (long long)make_layout(d, nullptr, nullptr, true, true).scratch_floats;
    return 0;
}

// part: 0 whole block, 1 up to the max over the ball (the per-point tail is left to cmf_setconv_tail_forward)
static int setconv_forward_part(const cmf_setconv_desc *d, void *st, int part)
{
    CMF_CHECK_ARG(d && d->xyz && d->y && d->wx && d->saved && d->scratch && d->out);
    CMF_CHECK_ARG(!gather_layout(d) || gather_operands_aligned(d));
    const Layout L = make_layout(d, d->saved, d->scratch, false);
    const long long P = (long long)d->B * d->N, M = P * d->S;
    const int O1 = d->O1, C2 = d->C[0], C3 = d->C[1];
    const Bn &b0 = L.bn[0], &b2 = L.bn[2];
    // idx is pre-zeroed like the reference's BallQuery.forward (every point is its own neighbour here, but keep the contract)
    if (!d->training) CMF_TRY(fold_all_eval(d, L, st));
    if (!d->idx_ready) CMF_TRY(cmf_ball_query_defined(d->B, d->N, d->N, d->radius, d->S, d->xyz, d->xyz, L.idx, st));
    // Three ways to the pooled rows L.x; the per-point tail behind them is the same sequence for all (eval mode: its folds are no-ops).
    if (setconv_path(d) == 1) {
        // inference of the narrow block (first encoder): layers 1-3 and the max over the ball as ONE register-chain kernel
        // (csrc/setconv_chain.hip; every layer bit-identical to the per-layer kernels) -- nothing but the pooled rows is written
        CMF_TRY(cmf_setconv_chain_infer(M, d->N, d->S, L.idx, d->xyz, d->y, d->ldy, d->wx, d->ldwx, L.bn[0].block(), L.bn[1].block(),
                                        L.bn[2].block(), d->w[0], d->w[1], L.x, C3, st));
    } else if (chain_train(d)) {
        // eval-mode BN with a backward pass to follow (one pass): nothing but the pooled rows, their argmax slots and the selected
        // pre-activations is stored
        CMF_TRY(cmf_setconv_chain_pass(1, M, d->N, d->S, L.idx, d->xyz, d->y, d->ldy, d->wx, d->ldwx, L.bn[0].block(), L.bn[1].block(),
                                       L.bn[2].block(), d->w[0], d->w[1], L.x, C3, L.z3, L.argmax, L.partial, nullptr, nullptr, nullptr, nullptr, st));
    } else {
        // gathering first layer: the grouped tensor z1 (M x O1: 1 GB at the largest scale of the second encoder) is never written -- the
        // second layer's GEMM gathers the per-point rows and forms the layer in its A-operand path (cmf_gemm_gather_affine, bit-identical);
        // the slot of z1 holds the M source-row indices and the coordinate planes of Wx.  Training on the compact layout (gather_layout),
        // or inference (eval-mode BN and no backward call to follow) on shapes the kernel takes.
        const bool gather = gather_layout(d) || (!d->training && d->inference && M % 128 == 0 && C2 % 128 == 0 && O1 % 16 == 0 &&
                                                 d->ldy % 4 == 0 && gather_operands_aligned(d) && M < (1ll << 31));
        if (gather) {
            if (d->training) {                          // the layer's statistics from cmf_group_affine's statistics-only form
                CMF_TRY(cmf_group_affine(d->B, d->N, d->N, d->S, O1, d->y, (int)d->ldy, nullptr, 0, d->xyz, d->xyz, d->wx, (int)d->ldwx, L.idx, 0,
                                         nullptr, L.dxyz, L.partial, L.partial_x, st));
                CMF_TRY(cmf_colsum(tiles128(M), 3 * O1 + 4, L.partial_x, L.fwd_sums, 0, nullptr, nullptr, st));
                CMF_TRY(fold(d, L, 0, st));
            }
            CMF_TRY(cmf_group_prep(d->B, d->N, d->N, d->S, O1, d->xyz, d->xyz, d->wx, (int)d->ldwx, L.idx, gather_rows(L), L.dxyz,
                                   gather_wx3(L, M), st));
            CMF_TRY(cmf_gemm_gather_affine((int)M, C2, O1, d->y, d->ldy, gather_rows(L), L.dxyz, gather_wx3(L, M), b0.a, b0.c, d->w[0], O1,
                                           L.z2, C2, d->training ? L.partial : nullptr, st));
        } else {
            CMF_TRY(cmf_group_affine(d->B, d->N, d->N, d->S, O1, d->y, (int)d->ldy, nullptr, 0, d->xyz, d->xyz, d->wx, (int)d->ldwx, L.idx, 0,
                                     L.z1, L.dxyz, d->training ? L.partial : nullptr, d->training ? L.partial_x : nullptr, st));
            if (d->training) CMF_TRY(cmf_colsum(tiles128(M), 3 * O1 + 4, L.partial_x, L.fwd_sums, 0, nullptr, nullptr, st));
            CMF_TRY(fold(d, L, 0, st));
            CMF_TRY(fwd_gemm(fwd_layer(d, L, 1), st));
        }
        CMF_TRY(fold(d, L, 1, st));
        CMF_TRY(fwd_gemm(fwd_layer(d, L, 2), st));
        CMF_TRY(fold(d, L, 2, st));
        CMF_TRY(cmf_bn_relu_maxpool_sel(P, d->S, C3, L.z3, b2.a, b2.c, L.x, C3, L.argmax, L.zsel, st));
    }
    return part == 1 ? 0 : forward_tail(d, L, st);
}

extern "C" int cmf_setconv_forward(const cmf_setconv_desc *d, void *st) { return setconv_forward_part(d, st, 0); }

// the way cmf_setconv_forward / _backward take for this descriptor (setconv_path above; shape fields, d->training, d->inference, d->ldy
// and the alignment of d->y are read, nothing is launched)
extern "C" int cmf_setconv_path(const cmf_setconv_desc *d) { return d ? setconv_path(d) : 0; }

// counts: NULL (dense), or per block the device array (B) int32 of its samples' point counts (ragged samples: cmf_setconv_queries_counted)
static int setconv_queries(int n, const cmf_setconv_desc *descs, const int *const *counts, void *stream)
{
    CMF_CHECK_ARG(n >= 0 && (n == 0 || descs));
    int i = 0;
    while (i < n) {
        // a run of blocks over the same cloud (the scales of one encoder call), then -- if the next run has the same shape -- a second cloud
        const cmf_setconv_desc &d0 = descs[i];
        CMF_CHECK_ARG(d0.xyz && d0.saved);
        int nq = 1;
        while (i + nq < n && nq < 4 && descs[i + nq].xyz == d0.xyz && descs[i + nq].B == d0.B && descs[i + nq].N == d0.N) ++nq;
        int nclouds = 1;
        if (i + 2 * nq <= n && descs[i + nq].xyz != d0.xyz && descs[i + nq].B == d0.B && descs[i + nq].N == d0.N) {
            bool same = true;
            for (int q = 0; q < nq && same; ++q) {
                const cmf_setconv_desc &u = descs[i + q], &v = descs[i + nq + q];
                same = v.xyz == descs[i + nq].xyz && v.radius == u.radius && v.S == u.S && v.B == u.B && v.N == u.N;
            }
            if (same) nclouds = 2;
        }
        int ns_chk[4];
        for (int q = 0; q < nq; ++q) ns_chk[q] = descs[i + q].S;
        if (counts) {                                         // ragged samples: the nested one-scan query only (n <= 1024), never an uncounted path
            CMF_CHECK_ARG(cmf_ball_query_multi_takes(d0.N, nq, ns_chk));
            for (int q = 0; q < nq * nclouds; ++q) CMF_CHECK_ARG(counts[i + q] && counts[i + q] == counts[i + (q / nq) * nq]);
        }
        if (!cmf_ball_query_multi_takes(d0.N, nq, ns_chk)) {  // large clouds (cell grid) / lists too long for one launch: the single-scale queries
            for (int q = 0; q < nq * nclouds; ++q) {
                const cmf_setconv_desc &d = descs[i + q];
                const Layout L = make_layout(&d, d.saved, nullptr, false);
                CMF_TRY(cmf_ball_query_defined(d.B, d.N, d.N, d.radius, d.S, d.xyz, d.xyz, L.idx, stream));
            }
        } else {
            float radii[4];
            int ns[4];
            const float *ctr[2], *cloud[2];
            int *idx[8];
            for (int c = 0; c < nclouds; ++c) {
                ctr[c] = cloud[c] = descs[i + c * nq].xyz;
                for (int q = 0; q < nq; ++q) {
                    const cmf_setconv_desc &d = descs[i + c * nq + q];
                    CMF_CHECK_ARG(d.saved);
                    idx[c * nq + q] = make_layout(&d, d.saved, nullptr, false).idx;
                    if (c == 0) { radii[q] = d.radius; ns[q] = d.S; }
                }
            }
            if (counts) {
                const int *cnt[2] = {counts[i], counts[i + (nclouds - 1) * nq]};
                CMF_TRY(cmf_ball_query_multi_counted(d0.B, d0.N, d0.N, nq, radii, ns, nclouds, ctr, cloud, idx, cnt, cnt, stream));
            } else
                CMF_TRY(cmf_ball_query_multi(d0.B, d0.N, d0.N, nq, radii, ns, nclouds, ctr, cloud, idx, 1, stream));
        }
        i += nq * nclouds;
    }
    return 0;
}

extern "C" int cmf_setconv_queries(int n, const cmf_setconv_desc *descs, void *stream) { return setconv_queries(n, descs, nullptr, stream); }

extern "C" int cmf_setconv_queries_counted(int n, const cmf_setconv_desc *descs, const int *const *counts, void *stream)
{
    CMF_CHECK_ARG(n == 0 || counts);
    return setconv_queries(n, descs, counts, stream);
}

// ---- the per-point tails of n blocks in batched launches (cmf_common.h "batched launches") ---------------------------
// Layers 4-6 of a block work on B*N rows of <= 64 channels: 128 workgroups of latency per kernel.  The blocks of an
// encoder call (4 scales, or 2 x 4 for the two clouds of the first encoder) run them as ONE launch per kernel of the
// sequence below -- the same kernels in the same order as cmf_setconv_forward / _backward, so results are bit-identical.
static bool tail_batchable(int n, const cmf_setconv_desc *descs)
{
    if (!tail_batch_on() || n < 1 || n > CMF_MAX_BATCH) return false;
    for (int i = 0; i < n; ++i) {
        const cmf_setconv_desc &d = descs[i];
        for (int k = 1; k < 5; ++k)
            if (d.C[k] > 64 || d.C[k] % 32 || d.C[k] != descs[0].C[k]) return false;
        if (d.training != descs[0].training || ((long long)d.B * d.N) % 128) return false;
        for (int k = 2; k < 5; ++k) if (!d.dw[k] && descs[0].dw[k]) return false;
    }
    return true;
}

extern "C" int cmf_setconv_tail_forward(int n, const cmf_setconv_desc *descs, void *stream)
{
    CMF_CHECK_ARG(n >= 0 && (n == 0 || descs));
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (!tail_batchable(n, descs)) {                    // one block after the other, unbatched kernels
        for (int i = 0; i < n; ++i) CMF_TRY(forward_tail(&descs[i], make_layout(&descs[i], descs[i].saved, descs[i].scratch, false), stream));
        return 0;
    }
    Layout L[CMF_MAX_BATCH];
    for (int i = 0; i < n; ++i) L[i] = make_layout(&descs[i], descs[i].saved, descs[i].scratch, false);
    for (int l = 3; l < 6; ++l) {
        GemmArgs g[CMF_MAX_BATCH];
        CmfBnFinArgs f[CMF_MAX_BATCH];
        for (int i = 0; i < n; ++i) {
            g[i] = fwd_layer(&descs[i], L[i], l);
            f[i] = fold_args(&descs[i], L[i], l);
        }
        CMF_TRY(cmf_thin_fwd_batch(n, g, st));
        if (descs[0].training) CMF_TRY(cmf_bn_finalize_batch(n, f, st));
    }
    CmfAffineArgs a[CMF_MAX_BATCH];
    for (int i = 0; i < n; ++i) a[i] = out_args(&descs[i], L[i]);
    return cmf_affine_relu_batch(n, a, st);
}

// gradient of the tails: from dout to the gradient of the pooled features (Layout::dx), with the weight / BN gradients of
// layers 4-6; the rest of each block's backward is cmf_setconv_backward with part 2
extern "C" int cmf_setconv_tail_backward(int n, const cmf_setconv_desc *descs, void *stream)
{
    CMF_CHECK_ARG(n >= 0 && (n == 0 || descs));
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (!tail_batchable(n, descs)) {
        for (int i = 0; i < n; ++i)
            CMF_TRY(backward_tail(&descs[i], make_layout(&descs[i], descs[i].saved, descs[i].scratch, true, descs[i].dy != nullptr), stream));
        return 0;
    }
    Layout L[CMF_MAX_BATCH];
    for (int i = 0; i < n; ++i) L[i] = make_layout(&descs[i], descs[i].saved, descs[i].scratch, true, descs[i].dy != nullptr);
    {
        CmfActBwdArgs a[CMF_MAX_BATCH];
        for (int i = 0; i < n; ++i) a[i] = dout_args(&descs[i], L[i]);
        CMF_TRY(cmf_act_bwd_stats_batch(n, a, st));
    }
    for (int l = 5; l >= 3; --l) {
        CmfColsumArgs cs[CMF_MAX_BATCH];
        CmfThinBwdCall tb[CMF_MAX_BATCH];
        CmfSplitkArgs sk[CMF_MAX_BATCH];
        for (int i = 0; i < n; ++i) {
            tb[i] = bwd_layer_args(&descs[i], L[i], l);
            cs[i] = bn_grad_args(&descs[i], L[i], l, tiles128(tb[i].rows));
        }
        CMF_TRY(cmf_colsum_batch(n, cs, st));
        CMF_TRY(cmf_thin_bwd_layer_batch(n, tb, st));
        for (int i = 0; i < n; ++i) sk[i] = splitk_args(tb[i]);
        CMF_TRY(cmf_splitk_reduce_batch(n, sk, st));
    }
    return 0;
}

// part: 0 whole block, 2 everything behind the per-point tail (cmf_setconv_tail_backward has produced Layout::dx)
static int setconv_backward_part(const cmf_setconv_desc *d, void *st, int part)
{
    CMF_CHECK_ARG(d && d->xyz && d->saved && d->scratch && d->dout);
    CMF_CHECK_ARG(!gather_layout(d) || (d->y && gather_operands_aligned(d)));
    const Layout L = make_layout(d, d->saved, d->scratch, true, d->dy != nullptr);
    const long long P = (long long)d->B * d->N, M = P * d->S;
    const int O1 = d->O1, C2 = d->C[0], C3 = d->C[1];
    const Bn &b0 = L.bn[0];
    const bool chain = chain_train(d);
    const int wv = chain ? (int)cmf_setconv_chain_waves(M, 1) : 0;          // statistics rows of a chain pass
    // The inverse index of the grouping is only needed by the scatter at the very end, but its kernel wants most of a
    // CU's LDS (one workgroup per sample, 132 KB at N = 256): issued there it has to wait until a CU has drained the
    // GEMM workgroups of the other chains -- up to a tile's duration on the critical tail of the chain.  Issued first
    // it runs next to the small per-point kernels and is long done when the scatter needs it.
    if (d->dy) CMF_TRY(cmf_build_inverse_ps(d->B, d->N, d->N, d->S, L.idx, L.offsets, L.inv, st));
    if (part != 2) CMF_TRY(backward_tail(d, L, st));                         // l = 5 .. 3 (per point)
    // max over the ball, l = 2 .. 1 (per neighbour slot).  Where a fused kernel takes l = 2, the gradient of the pooled tensor is
    // kept per POINT (g, in L.dx's neighbour L.dU3) and expanded on the fly -- the [M, C3] matrix is neither written nor read.
    float *g = L.dU3;
    const CmfThinBwdCall q = bwd_layer_args(d, L, 2);
    const bool fused = thin_fused_on() && M % 128 == 0 && d->dw[1];
    if (chain) {
        // the chain's backward: the pooled gradient with the BN-backward sums of l = 2 from the selected pre-activations (kept in z3's slot),
        // then two passes that recompute the layers they differentiate (weight-gradient slabs per workgroup, statistics rows per wave)
        const float *bn0 = L.bn[0].block(), *bn1 = L.bn[1].block(), *bn2 = L.bn[2].block();
        const int nslab = wv / 4;
        CMF_TRY(pooled_grad_head(d, L, L.z3, st));
        CMF_TRY(cmf_setconv_chain_pass(2, M, d->N, d->S, L.idx, d->xyz, d->y, d->ldy, d->wx, d->ldwx, bn0, bn1, bn2, d->w[0], d->w[1],
                                       nullptr, 0, nullptr, L.argmax, L.partial, g, nullptr, L.dU2, L.splitk, st));
        if (d->dw[1]) CMF_TRY(cmf_splitk_reduce(C3, C2, nslab, L.splitk, d->dw[1], C2, d->acc_w[1], (hipStream_t)st));
        CMF_TRY(bn_grad_sums(bn_grad_args(d, L, 1, wv), st));
        CMF_TRY(cmf_setconv_chain_pass(3, M, d->N, d->S, L.idx, d->xyz, d->y, d->ldy, d->wx, d->ldwx, bn0, bn1, bn2, d->w[0], d->w[1],
                                       nullptr, 0, nullptr, nullptr, L.partial, nullptr, L.dU2, L.dU1, L.splitk, st));
        if (d->dw[0]) CMF_TRY(cmf_splitk_reduce(C2, O1, nslab, L.splitk, d->dw[0], O1, d->acc_w[0], (hipStream_t)st));
    } else {
        if (fused && cmf_thin_bwd_supported(C3, C2) && C3 % 32 == 0 && C2 % 32 == 0) {                  // narrow layers
            CMF_TRY(pooled_grad_head(d, L, L.zsel, st));
            CMF_TRY(cmf_thin_bwd_layer_pooled(P, d->S, q.cout, q.cin, g, L.argmax, q.z, q.a, q.mean, q.invstd, q.sums, q.w, q.x, q.a_in, q.c_in,
                                              q.mean_in, q.invstd_in, q.dx, q.stats, q.dw, q.accumulate, q.slabs, st));
        } else if (fused && thin_wide_on() && cmf_thin_bwd_wide_supported(C3, C2)) {
            // 64 <- 256 channels (second encoder): the same single pass, a workgroup per (row range, 128 input channels).  CMF_THIN_WIDE=0
            // keeps max-pool backward, BN backward and the two tiled GEMMs (A/B: 22.6 vs 22.9 ms per step)
            CMF_TRY(pooled_grad_head(d, L, L.zsel, st));
            CMF_TRY(cmf_thin_bwd_wide_layer(q.rows, q.cin, nullptr, q.lddu, g, L.argmax, d->S, q.z, q.ldz, q.a, q.mean, q.invstd, q.sums, q.w, q.ldw,
                                            q.x, q.ldx, q.a_in, q.c_in, q.mean_in, q.invstd_in, q.dx, q.lddx, q.stats, q.dw, q.lddw, q.accumulate,
                                            q.slabs, st));
        } else {
            const Bn &b2 = L.bn[2];
            CMF_TRY(cmf_maxpool_bwd(P, d->S, C3, L.dx, C3, L.z3, b2.a, b2.c, b2.mean, b2.invstd, L.argmax, L.dU3, L.partial, st));
            CMF_TRY(bwd_layer(d, L, 2, st));
        }
        CMF_TRY(gather_layout(d) ? bwd_layer1_gather(d, L, st) : bwd_layer(d, L, 1, st));
    }
    // first layer: sums {s1,s2,q0,q1,q2}; dgamma/dbeta; dW_xyz from sums; BN backward folded into the scatter
    CMF_TRY(bn_grad_sums(bn_grad_args(d, L, 0, chain ? wv : tiles128(M)), st));       // (the statistics rows of the pass that formed dU1)
    const float *sums = d->training ? L.sums : nullptr;
    const float inv_count = (float)(1.0 / (double)M);
    if (d->dwx)
        CMF_TRY(cmf_setconv_dwx(O1, inv_count, d->training, L.sums, L.fwd_sums, b0.a, b0.mean, b0.invstd, d->dwx, (int)d->lddwx, d->acc_wx, st));
    if (d->dy) {
        // z1 rows of one source point differ only by wx . dxyz: the BN-backward part of the scatter has a closed form,
        // so only dU1 (or its pieces, summed inside the GEMM) is streamed (csrc/group_rows.hip)
        const int lddy = d->lddy ? (int)d->lddy : O1;
        if (gather_sum_layout(d))
            CMF_TRY(cmf_group_rows_grad_bn_cf_pieces(d->B, d->N, O1, d->N * d->S, d->S, sum_slots(d, L).pieces, d->y, d->ldy, d->wx, d->ldwx, d->xyz,
                                                     d->xyz, b0.a, b0.mean, b0.invstd, sums, inv_count, L.offsets, L.inv, d->dy, lddy, st));
        else
            CMF_TRY(cmf_group_rows_grad_bn_cf(d->B, d->N, O1, d->N * d->S, d->S, L.dU1, d->y, d->ldy, d->wx, d->ldwx, d->xyz, d->xyz, b0.a, b0.mean,
                                              b0.invstd, sums, inv_count, L.offsets, L.inv, d->dy, lddy, st));
    }
    return 0;
}

extern "C" int cmf_setconv_backward(const cmf_setconv_desc *d, void *st) { return setconv_backward_part(d, st, 0); }

// ---------------------------------------------------------------------------------------------------------------
// The independent scales of a MultiScaleEncoder (radarflow_util.py:101-118) in ONE call: descs[i] is issued on
// streams[i] from its own host thread.  At N = 256 a scale's ~20 (forward) / ~45 (backward) kernels run about as long
// as they take to enqueue, so one host thread cannot keep four streams fed.  Stream ordering against the
// caller's stream is the caller's business (events before / after the call); nothing is synchronised here.
// ---------------------------------------------------------------------------------------------------------------
namespace {
// Persistent host threads for the chains of a multi-scale call: a chain is ~20 / ~45 launches, i.e. a few hundred
// microseconds of enqueueing -- creating and joining a std::thread per chain and call (up to 7 spawns, ~6 calls per step)
// costs a comparable amount.  Workers are created on first use, sleep on a condition variable between calls and are
// never destroyed (the pool is leaked on purpose: joining threads during static destruction races with the HIP
// runtime's own teardown).
struct ChainWorker {
    std::mutex m;
    std::condition_variable cv;
    std::function<void()> job;
    bool pending = false, done = true;
    void loop()
    {
        for (;;) {
            std::function<void()> j;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return pending; });
                j = std::move(job);
                pending = false;
            }
            j();
            {
                std::lock_guard<std::mutex> lk(m);
                done = true;
            }
            cv.notify_all();
        }
    }
    void submit(std::function<void()> j)
    {
        {
            std::lock_guard<std::mutex> lk(m);
            job = std::move(j);
            pending = true;
            done = false;
        }
        cv.notify_all();
    }
    void wait()
    {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return done; });
    }
};
std::mutex g_pool_mutex;                                 // one multi-scale call at a time uses the pool
std::vector<ChainWorker *> *g_pool = nullptr;

ChainWorker *chain_worker(size_t i)
{
    if (!g_pool) g_pool = new std::vector<ChainWorker *>();
    while (g_pool->size() <= i) {
        ChainWorker *w = new ChainWorker();
        std::thread(&ChainWorker::loop, w).detach();
        g_pool->push_back(w);
    }
    return (*g_pool)[i];
}
}  // namespace

static int setconv_multi(int n, const cmf_setconv_desc *descs, void *const *streams, bool backward, int part = 0)
{
    CMF_CHECK_ARG(n >= 0 && n <= 16 && (n == 0 || (descs && streams)));
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return (int)hipGetLastError();
    int err[16] = {0};
    auto run = [&](int i) {
        if (i > 0 && hipSetDevice(dev) != hipSuccess) { err[i] = (int)hipGetLastError(); return; }
        err[i] = backward ? setconv_backward_part(&descs[i], streams[i], part) : setconv_forward_part(&descs[i], streams[i], part);
    };
    bool one_stream = true;                                 // every chain on the same stream (serialised diagnostic runs):
    for (int i = 1; i < n; ++i) one_stream = one_stream && streams[i] == streams[0];    // nothing to feed in parallel
    if (one_stream) {
        for (int i = 0; i < n; ++i) run(i);
    } else {
        std::lock_guard<std::mutex> pool_lock(g_pool_mutex);
        for (int i = 1; i < n; ++i) chain_worker((size_t)i - 1)->submit([&run, i] { run(i); });
        if (n > 0) run(0);                                  // the calling thread takes the first scale
        for (int i = 1; i < n; ++i) chain_worker((size_t)i - 1)->wait();
    }
    for (int i = 0; i < n; ++i) if (err[i]) return err[i];
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// The slot-level bodies of up to CMF_MAX_BATCH NARROW blocks (the first encoder: 2 clouds x 4 scales, 32 / 32 / 64 channels) in lock
// step: one batched launch per stage for all blocks instead of one kernel per block and stage on the stream pool.  At these widths
// every kernel of a body is an HBM stream of 15-70 us -- eight chains of eight launches each kept four hardware queues busy with
// launch gaps, and co-running bought nothing (the bodies' wall time equalled the sum of their kernels' isolated durations).  Same
// kernels' device code, same arithmetic, same results as the per-block calls.  Train-mode BatchNorm only (eval-mode BN takes the
// register chain); CMF_BODY_BATCH=0: the per-block chains (A/B).
// ---------------------------------------------------------------------------------------------------------------
static bool body_batchable(int n, const cmf_setconv_desc *descs)
{
    if (!body_batch_on() || n < 2 || n > CMF_MAX_BATCH) return false;
    for (int i = 0; i < n; ++i) {
        const cmf_setconv_desc &d = descs[i];
        const long long M = (long long)d.B * d.N * d.S;
        if (!d.training || d.inference || !d.idx_ready || gather_layout(&d)) return false;
        if (d.O1 != descs[0].O1 || d.C[0] != descs[0].C[0] || d.C[1] != descs[0].C[1]) return false;
        if (d.O1 > 64 || d.O1 % 32 || d.C[0] > 64 || d.C[0] % 32 || d.C[1] > 64 || d.C[1] % 32) return false;
        if (M % 128 || M >= (1ll << 31) || d.ldy % 4 || ((uintptr_t)d.y & 15)) return false;
    }
    return true;
}

// inference of the narrow blocks (eval-mode BN, no backward call to follow): their register-chain kernels as ONE launch
static bool infer_batchable(int n, const cmf_setconv_desc *descs)
{
    if (!body_batch_on() || n < 2 || n > CMF_MAX_BATCH) return false;
    for (int i = 0; i < n; ++i) {
        const cmf_setconv_desc &d = descs[i];
        const long long M = (long long)d.B * d.N * d.S;
        if (setconv_path(&d) != 1 || !d.idx_ready || M >= (1ll << 31)) return false;
        for (int l = 0; l < 6; ++l) if (!d.rmean[l] || !d.rvar[l]) return false;
    }
    return true;
}

static int setconv_infer_bodies_batch(int n, const cmf_setconv_desc *descs, hipStream_t st)
{
    CmfBatch<FoldAll> fb;
    CmfChainInferArgs q[CMF_MAX_BATCH];
    for (int i = 0; i < n; ++i) {
        const cmf_setconv_desc &d = descs[i];
        CMF_CHECK_ARG(d.xyz && d.y && d.wx && d.saved && d.scratch && d.out);
        const Layout L = make_layout(&d, d.saved, d.scratch, false);
        fb.a[i] = fold_all_args(&d, L);
        q[i] = CmfChainInferArgs{(long long)d.B * d.N * d.S, d.N, d.S, L.idx, d.xyz, d.y, d.ldy, d.wx, d.ldwx, L.bn[0].block(), L.bn[1].block(),
                                 L.bn[2].block(), d.w[0], d.w[1], L.x, d.C[1]};
    }
    hipLaunchKernelGGL(bn_fold_eval_batch_kernel, dim3(6, n), dim3(256), 0, st, fb);
    CMF_TRY(cmf_launch_status());
    return cmf_setconv_chain_infer_batch(n, q, st);
}

// largest block first: blockIdx.y = block and the dispatcher walks y slowest, so the blocks with the most rows start first and the small
// ones fill the tail of the launch
static void largest_first(int n, const cmf_setconv_desc *in, cmf_setconv_desc *out)
{
    int ord[CMF_MAX_BATCH];
    for (int i = 0; i < n; ++i) ord[i] = i;
    std::stable_sort(ord, ord + n, [&](int a, int b) { return (long long)in[a].B * in[a].N * in[a].S > (long long)in[b].B * in[b].N * in[b].S; });
    for (int i = 0; i < n; ++i) out[i] = in[ord[i]];
}

static int setconv_forward_bodies_batch(int n, const cmf_setconv_desc *descs_in, hipStream_t st)
{
    cmf_setconv_desc descs[CMF_MAX_BATCH];
    largest_first(n, descs_in, descs);
    Layout L[CMF_MAX_BATCH];
    for (int i = 0; i < n; ++i) {
        CMF_CHECK_ARG(descs[i].xyz && descs[i].y && descs[i].wx && descs[i].saved && descs[i].scratch && descs[i].out);
        L[i] = make_layout(&descs[i], descs[i].saved, descs[i].scratch, false);
    }
    const int O1 = descs[0].O1, C3 = descs[0].C[1];
    {   // z1 = y[idx] + Wx . dxyz with its statistics; the z * d_k sums for dW_xyz
        CmfGroupAffineArgs ga[CMF_MAX_BATCH];
        CmfColsumArgs cs[CMF_MAX_BATCH];
        for (int i = 0; i < n; ++i) {
            const cmf_setconv_desc &d = descs[i];
            const long long M = (long long)d.B * d.N * d.S;
            ga[i] = CmfGroupAffineArgs{d.B, d.N, d.N, d.S, O1, d.y, (int)d.ldy, d.xyz, d.xyz, d.wx, (int)d.ldwx, L[i].idx, L[i].z1, L[i].dxyz,
                                       L[i].partial, L[i].partial_x};
            cs[i] = CmfColsumArgs{tiles128(M), 3 * O1 + 4, L[i].partial_x, L[i].fwd_sums, 0, nullptr, nullptr, 0};
        }
        CMF_TRY(cmf_group_affine_batch(n, ga, st));
        CMF_TRY(cmf_colsum_batch(n, cs, st));
    }
    for (int l = 0; l < 3; ++l) {                        // fold BN layer l, then (l = 0, 1) the next 1x1 conv / (l = 2) the max over the ball
        CmfBnFinArgs f[CMF_MAX_BATCH];
        GemmArgs g[CMF_MAX_BATCH];
        CmfPoolArgs pl[CMF_MAX_BATCH];
        for (int i = 0; i < n; ++i) {
            const cmf_setconv_desc &d = descs[i];
            const Bn &b = L[i].bn[l];
            f[i] = fold_args(&d, L[i], l);
            if (l < 2) g[i] = fwd_layer(&d, L[i], l + 1);
            else pl[i] = CmfPoolArgs{(long long)d.B * d.N, d.S, C3, L[i].z3, b.a, b.c, L[i].x, C3, L[i].argmax, 0, L[i].zsel};
        }
        CMF_TRY(cmf_bn_finalize_batch(n, f, st));
        if (l < 2) CMF_TRY(cmf_thin_fwd_batch(n, g, st));
        else CMF_TRY(cmf_bn_relu_maxpool_batch(n, pl, st));
    }
    return 0;
}

// backward of the same bodies (behind cmf_setconv_tail_backward, which has produced Layout::dx): the kernels of setconv_backward_part's
// narrow path, one batched launch per stage
static bool body_batchable_bwd(int n, const cmf_setconv_desc *descs)
{
    if (!body_batchable(n, descs)) return false;
    for (int i = 0; i < n; ++i) {
        const cmf_setconv_desc &d = descs[i];
        if (!thin_fused_on() || !d.dw[0] || !d.dw[1] || !d.dout || !cmf_thin_bwd_supported(d.C[1], d.C[0]) || !cmf_thin_bwd_supported(d.C[0], d.O1)) return false;
        if (d.C[1] != 64 || d.C[0] != 32 || d.O1 != 32) return false;                 // the batched instantiations of the fused layer
        if ((d.dy != nullptr) != (descs[0].dy != nullptr) || (d.dwx != nullptr) != (descs[0].dwx != nullptr)) return false;
        if (d.B != descs[0].B || d.N != descs[0].N || d.N > 256 || d.S > 64) return false;
    }
    return true;
}

static int splitk_batch_or_each(int n, const CmfSplitkArgs *sk, hipStream_t st)
{
    if (cmf_splitk_reduce_batch(n, sk, st) == 0) return 0;          // (refused without a launch when the problems want different kernels)
    (void)hipGetLastError();
    for (int i = 0; i < n; ++i) CMF_TRY(cmf_splitk_reduce(sk[i].M, sk[i].N, sk[i].split_k, sk[i].workspace, sk[i].C, sk[i].ldc, sk[i].accumulate, st));
    return 0;
}

static int setconv_backward_bodies_batch(int n, const cmf_setconv_desc *descs_in, hipStream_t st)
{
    cmf_setconv_desc descs[CMF_MAX_BATCH];
    largest_first(n, descs_in, descs);
    Layout L[CMF_MAX_BATCH];
    for (int i = 0; i < n; ++i) {
        CMF_CHECK_ARG(descs[i].xyz && descs[i].saved && descs[i].scratch && descs[i].dout);
        L[i] = make_layout(&descs[i], descs[i].saved, descs[i].scratch, true, descs[i].dy != nullptr);
    }
    const int O1 = descs[0].O1, C3 = descs[0].C[1];
    const bool want_dy = descs[0].dy != nullptr, want_dwx = descs[0].dwx != nullptr;
    if (want_dy) {
        CmfInverseArgs iv[CMF_MAX_BATCH];
        for (int i = 0; i < n; ++i) iv[i] = CmfInverseArgs{descs[i].N, descs[i].N, descs[i].S, L[i].idx, L[i].offsets, L[i].inv};
        CMF_TRY(cmf_build_inverse_ps_batch(n, descs[0].B, iv, st));
    }
    CmfColsumArgs cs[CMF_MAX_BATCH];
    CmfThinBwdCall tb[CMF_MAX_BATCH];
    CmfSplitkArgs sk[CMF_MAX_BATCH];
    for (int l = 2; l >= 1; --l) {
        // l = 2: max over the ball -> the pooled gradient per point (g) with the layer's BN-backward sums, then the layer (64 <- 32) from
        // the pooled gradient; l = 1: the layer (32 <- 32) with the dxyz sums of the first layer's coordinate weights
        CmfPoolBwdArgs pb[CMF_MAX_BATCH];
        for (int i = 0; i < n; ++i) {
            const cmf_setconv_desc &d = descs[i];
            CmfThinBwdCall &q = tb[i];
            q = bwd_layer_args(&d, L[i], l);
            cs[i] = bn_grad_args(&d, L[i], l, tiles128(l == 2 ? rows_of(&d, 3) : q.rows));      // (l = 2: partials per point)
            if (l == 2) {
                const Bn &b2 = L[i].bn[2];
                float *g = L[i].dU3;
                pb[i] = CmfPoolBwdArgs{rows_of(&d, 3), d.S, C3, L[i].dx, C3, L[i].zsel, b2.a, b2.c, b2.mean, b2.invstd, L[i].argmax, g, L[i].partial, 1};
                q.dU = nullptr; q.pool_g = g; q.pool_am = L[i].argmax; q.pool_S = d.S;
            }
        }
        if (l == 2) CMF_TRY(cmf_maxpool_bwd_point_batch(n, pb, st));
        CMF_TRY(cmf_colsum_batch(n, cs, st));
        CMF_TRY(cmf_thin_bwd_layer_batch(n, tb, st));
        for (int i = 0; i < n; ++i) sk[i] = splitk_args(tb[i]);
        CMF_TRY(splitk_batch_or_each(n, sk, st));
    }
    {   // first layer: sums {s1, s2, q0, q1, q2}; dgamma / dbeta; dW_xyz; BN backward folded into the scatter
        CmfDwxArgs dx[CMF_MAX_BATCH];
        CmfScatterArgs sc[CMF_MAX_BATCH];
        for (int i = 0; i < n; ++i) {
            const cmf_setconv_desc &d = descs[i];
            const long long M = rows_of(&d, 0);
            const float inv_count = (float)(1.0 / (double)M);
            const Bn &b0 = L[i].bn[0];
            cs[i] = bn_grad_args(&d, L[i], 0, tiles128(M));
            dx[i] = CmfDwxArgs{O1, inv_count, d.training, L[i].sums, L[i].fwd_sums, b0.a, b0.mean, b0.invstd, d.dwx, (int)d.lddwx, d.acc_wx};
            sc[i] = CmfScatterArgs{d.N, d.N * d.S, d.S, L[i].dU1, d.y, d.ldy, d.wx, d.ldwx, d.xyz, d.xyz, b0.a, b0.mean, b0.invstd, L[i].sums,
                                   inv_count, L[i].offsets, L[i].inv, d.dy, d.lddy ? (int)d.lddy : O1};
        }
        CMF_TRY(cmf_colsum_batch(n, cs, st));
        if (want_dwx) CMF_TRY(cmf_setconv_dwx_batch(n, dx, st));
        if (want_dy) CMF_TRY(cmf_group_rows_grad_bn_cf_batch(n, descs[0].B, O1, sc, st));
    }
    return 0;
}

// 1 when cmf_setconv_backward_bodies_multi will run these blocks' bodies as batched launches on streams[0] alone, else 0
extern "C" int cmf_setconv_backward_bodies_batched(int n, const cmf_setconv_desc *descs)
{
    return (n >= 0 && n <= 16 && descs && body_batchable_bwd(n, descs)) ? 1 : 0;
}

// The same with the per-point tails taken out: forward stops behind the max over the ball, backward starts there.  The
// caller runs cmf_setconv_tail_forward behind the forward heads (after joining the streams) and cmf_setconv_tail_backward in
// front of the backward bodies (before forking): the tails of all blocks as batched launches on one stream.
// 1 when cmf_setconv_forward_heads_multi will run these blocks' bodies as batched launches on streams[0] alone (the caller may then pass
// its own stream for every entry and skip the fork / join around the call), else 0
extern "C" int cmf_setconv_forward_bodies_batched(int n, const cmf_setconv_desc *descs)
{
    return (n >= 0 && n <= 16 && descs && (body_batchable(n, descs) || infer_batchable(n, descs))) ? 1 : 0;
}

// The batched forms run every block on streams[0].  A caller that prepared block i's inputs on streams[i] (the contract of the
// per-chain form: INTEGRATION.md "fork / join") is still ordered: streams[0] waits for what is queued on every other distinct stream
// before the batched launches, and those streams wait for streams[0] behind them.  With all entries equal (the Python host, which asks
// cmf_setconv_*_bodies_batched first) nothing is recorded.
static int batched_order(int n, void *const *streams, bool before)
{
    hipStream_t s0 = (hipStream_t)streams[0];
    hipEvent_t back = nullptr;
    for (int i = 1; i < n; ++i) {
        hipStream_t si = (hipStream_t)streams[i];
        if (si == s0) continue;
        bool seen = false;
        for (int j = 1; j < i; ++j) seen = seen || streams[j] == streams[i];
        if (seen) continue;
        if (before) {
            hipEvent_t ev;
            if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return (int)hipGetLastError();
            if (hipEventRecord(ev, si) != hipSuccess || hipStreamWaitEvent(s0, ev, 0) != hipSuccess) { (void)hipEventDestroy(ev); return (int)hipGetLastError(); }
            (void)hipEventDestroy(ev);                  // (released by the runtime once the recorded work has completed)
        } else {
            if (!back) {
                if (hipEventCreateWithFlags(&back, hipEventDisableTiming) != hipSuccess) return (int)hipGetLastError();
                if (hipEventRecord(back, s0) != hipSuccess) { (void)hipEventDestroy(back); return (int)hipGetLastError(); }
            }
            if (hipStreamWaitEvent(si, back, 0) != hipSuccess) { (void)hipEventDestroy(back); return (int)hipGetLastError(); }
        }
    }
    if (back) (void)hipEventDestroy(back);
    return 0;
}

extern "C" int cmf_setconv_forward_heads_multi(int n, const cmf_setconv_desc *descs, void *const *streams)
{
    CMF_CHECK_ARG(n >= 0 && n <= 16 && (n == 0 || (descs && streams)));
    const bool body = body_batchable(n, descs);
    if (body || infer_batchable(n, descs)) {
        CMF_TRY(batched_order(n, streams, true));
        CMF_TRY(body ? setconv_forward_bodies_batch(n, descs, (hipStream_t)streams[0]) : setconv_infer_bodies_batch(n, descs, (hipStream_t)streams[0]));
        return batched_order(n, streams, false);
    }
    return setconv_multi(n, descs, streams, false, 1);
}

extern "C" int cmf_setconv_backward_bodies_multi(int n, const cmf_setconv_desc *descs, void *const *streams)
{
    CMF_CHECK_ARG(n >= 0 && n <= 16 && (n == 0 || (descs && streams)));
    if (body_batchable_bwd(n, descs)) {
        CMF_TRY(batched_order(n, streams, true));
        CMF_TRY(setconv_backward_bodies_batch(n, descs, (hipStream_t)streams[0]));
        return batched_order(n, streams, false);
    }
    return setconv_multi(n, descs, streams, true, 2);
}

// ---------------------------------------------------------------------------------------------------------------
// [conv + BN + ReLU] x L on a materialised input (the heads' stacks): cmf_mlp_forward / _backward.  The kernel sequence
// of fused_blocks.MLPChainFn, issued from here.
// ---------------------------------------------------------------------------------------------------------------
namespace {
struct MlpLayout {
    float *z[4];
    Bn bn[4];
    float *partial, *sums, *dU[4], *splitk;
    size_t saved_floats, scratch_floats;
};
MlpLayout mlp_layout(const cmf_mlp_desc *d, float *saved, float *scratch, bool backward)
{
    MlpLayout L;
    Bump s(saved);
    for (int l = 0; l < d->L; ++l) L.z[l] = s.take((size_t)d->M * d->C[l + 1]);
    for (int l = 0; l < d->L; ++l) L.bn[l] = Bn(s.take(4 * (size_t)d->C[l + 1]), d->C[l + 1]);
    L.saved_floats = s.off;
    Bump t(scratch);
    int cmax = 0;
    for (int l = 0; l <= d->L; ++l) cmax = std::max(cmax, d->C[l]);
    L.partial = t.take((size_t)tiles128(d->M) * 2 * cmax);
    L.sums = t.take(2 * (size_t)cmax);
    size_t sk = 0;
    if (backward) {
        for (int l = 0; l < d->L; ++l) L.dU[l] = t.take((size_t)d->M * d->C[l + 1]);
        for (int l = 0; l < d->L; ++l) sk = std::max(sk, (size_t)dw_split(d->M, d->C[l + 1], d->C[l]) * d->C[l + 1] * d->C[l]);
        L.splitk = t.take(sk);
    } else {
        for (int l = 0; l < 4; ++l) L.dU[l] = nullptr;
        L.splitk = nullptr;
    }
    L.scratch_floats = t.off;
    return L;
}
bool mlp_ok(const cmf_mlp_desc *d)
{
    if (!d || d->M <= 0 || d->M >= (1ll << 31) || d->L < 1 || d->L > 4) return false;
    for (int l = 0; l <= d->L; ++l) if (d->C[l] <= 0 || d->C[l] % 4) return false;
    return true;
}
}  // namespace

extern "C" int cmf_mlp_sizes(const cmf_mlp_desc *d, long long *saved_floats, long long *scratch_fwd, long long *scratch_bwd)
{
    CMF_CHECK_ARG(mlp_ok(d));
    const MlpLayout f = mlp_layout(d, nullptr, nullptr, false), b = mlp_layout(d, nullptr, nullptr, true);
    if (saved_floats) *saved_floats = (long long)f.saved_floats;
    if (scratch_fwd) *scratch_fwd = (long long)f.scratch_floats;
    if (scratch_bwd) *scratch_bwd = (long long)b.scratch_floats;
    return 0;
}

extern "C" int cmf_mlp_forward(const cmf_mlp_desc *d, void *st)
{
    CMF_CHECK_ARG(mlp_ok(d) && d->x && d->saved && d->scratch && d->out && d->ldx % 4 == 0 && d->ldo % 4 == 0);
    const MlpLayout L = mlp_layout(d, d->saved, d->scratch, false);
    for (int l = 0; l < d->L; ++l) {
        const int cin = d->C[l], cout = d->C[l + 1];
        CMF_TRY(fwd_gemm(fwd_gemm_args(d->M, cin, cout, l == 0 ? d->x : L.z[l - 1], l == 0 ? d->ldx : cin, l > 0 ? L.bn[l - 1] : Bn(), d->w[l],
                                       L.z[l], d->training ? L.partial : nullptr), st));
        CmfBnFinArgs f = bn_fin_args(d, l, d->M, cout, L.partial, L.bn[l]);
        if (!d->training) { f.tiles = 0; f.count = 1.0; f.partial = nullptr; f.momentum = 0.f; f.nbt = nullptr; }      // fold the running statistics
        CMF_TRY(bn_finalize(f, st));
    }
    const int cl = d->C[d->L];
    return affine_relu(affine_args(d->M, cl, L.z[d->L - 1], L.bn[d->L - 1], d->out, d->ldo), st);
}

extern "C" int cmf_mlp_backward(const cmf_mlp_desc *d, void *st)
{
    CMF_CHECK_ARG(mlp_ok(d) && d->x && d->saved && d->scratch && d->dout && d->lddout % 4 == 0 && (!d->dx || d->lddx % 4 == 0));
    const MlpLayout L = mlp_layout(d, d->saved, d->scratch, true);
    const long long M = d->M;
    const int top = d->L - 1;
    CMF_TRY(act_bwd(act_bwd_args(M, d->C[d->L], d->dout, d->lddout, L.z[top], L.bn[top], L.dU[top], L.partial), st));
    for (int l = top; l >= 0; --l) {
        const int cin = d->C[l], cout = d->C[l + 1];
        const Bn &b = L.bn[l], in = l > 0 ? L.bn[l - 1] : Bn();
        CMF_CHECK_ARG(d->dw[l] && d->dgamma[l] && d->dbeta[l]);
        CMF_TRY(bn_grad_sums(bn_grad_args(d, l, tiles128(M), 2 * cout, cout, L.partial, L.sums), st));
        CMF_TRY(cmf_bn_bwd_apply(M, cout, L.dU[l], L.z[l], cout, b.a, b.mean, b.invstd, d->training ? L.sums : nullptr, st));
        // weight gradient dZ^T act(x_in); then the gradient w.r.t. the pre-activation of the layer below, masked, with its BN-backward
        // sums -- or, for the first layer, the plain gradient of the input when it is wanted
        CMF_TRY(dw_gemm(M, cout, cin, L.dU[l], l == 0 ? d->x : L.z[l - 1], l == 0 ? d->ldx : cin, in, d->dw[l], d->acc_w[l], L.splitk, st));
        if (l > 0) CMF_TRY(dx_gemm(M, cout, cin, L.dU[l], d->w[l], L.dU[l - 1], cin, L.z[l - 1], in, L.partial, nullptr, st));
        else if (d->dx) CMF_TRY(dx_gemm(M, cout, cin, L.dU[0], d->w[0], d->dx, d->lddx, nullptr, in, nullptr, nullptr, st));
    }
    return 0;
}

// Float offsets of the per-layer BatchNorm blocks (mean | invstd | a | c, 4*C_l floats each) inside `saved`.
extern "C" int cmf_setconv_bn_offsets(const cmf_setconv_desc *d, long long *offsets6)
{
    CMF_CHECK_ARG(d && offsets6);
    // lay the arena out over a fake non-null base (Bump hands out NULL for a NULL base) and subtract it again
    float *const fake = reinterpret_cast<float *>(uintptr_t(1) << 40);
    const Layout L = make_layout(d, fake, nullptr, false);
    for (int l = 0; l < 6; ++l) offsets6[l] = (long long)(L.bn[l].block() - fake);
    return 0;
}

// Deferred running-statistics update for encoder calls that ran concurrently (two clouds through the same weight-shared
// encoder, radarflow_util.py:111-118 called twice per step, cmflow.py:72-73): the block calls were issued with
// rmean == NULL (batch statistics only) and the nn.BatchNorm2d momentum update is applied here once per call, in call
// order, from the saved batch mean / invstd of each call.  One workgroup per table entry (= one BN layer of one scale).
__global__ __launch_bounds__(64) void bn_running_update_kernel(const cmf_bn_update_entry *__restrict__ table, int n_calls,
                                                              const float *__restrict__ saved0, const float *__restrict__ saved1)
{
    const cmf_bn_update_entry e = table[blockIdx.x];
    const double mo = e.momentum, cnt = e.count;
    for (int c = threadIdx.x; c < e.C; c += 64) {
        double rm = e.rmean[c], rv = e.rvar[c];
        for (int k = 0; k < n_calls; ++k) {
            const float *s = (k == 0 ? saved0 : saved1) + e.offset;
            const double mean = s[c], invstd = s[e.C + c];
            double var = 1.0 / (invstd * invstd) - (double)e.eps;
            if (var < 0.0) var = 0.0;
            const double unbiased = cnt > 1.0 ? var * cnt / (cnt - 1.0) : var;
            rm = (1.0 - mo) * rm + mo * mean;
            rv = (1.0 - mo) * rv + mo * unbiased;
        }
        e.rmean[c] = (float)rm; e.rvar[c] = (float)rv;
    }
    if (threadIdx.x == 0 && e.nbt) *e.nbt += n_calls;
}

extern "C" int cmf_bn_running_update(int n_entries, const cmf_bn_update_entry *table, int n_calls, const float *saved0,
                                     const float *saved1, void *stream)
{
    CMF_CHECK_ARG(n_entries >= 0 && n_calls >= 1 && n_calls <= 2 && (n_entries == 0 || (table && saved0 && (n_calls == 1 || saved1))));
    if (n_entries == 0) return 0;
    hipLaunchKernelGGL(bn_running_update_kernel, dim3(n_entries), dim3(64), 0, (hipStream_t)stream, table, n_calls, saved0, saved1);
    return cmf_launch_status();
}
