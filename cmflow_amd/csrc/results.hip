// What a test epoch leaves behind (cmflow_amd/results.py) -- the reference's `save_res` branch
// (main_util.py:149-168, clip_util.py:238-257) without its per-frame copies to the host.
//   cmf_pack_results: the valid rows of one ragged batch's outputs into the split-wide packed store, the inverse of cmf_draw_frames;
//   cmf_pose_chain:   the per-clip prefix product of the inverted per-frame transforms, the odometry result, as a DEFINITION:
//                     float64 from the float32 entries, a fixed operation order, every operation rounded on its own.
// (The per-frame metrics, cmf_eval_metrics_frames, sit in eval.hip next to the kernels they reuse.)
#include "cmf_common.h"
#include "../../include/cmflow_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int PACK_CHUNK = 256;

struct PackArgs {
    int B, N, F;
    long long total;                                                       // rows of the store, off1[F]
    const int *frames, *n1, *off1;
    const float *sf, *stat_cls;
    const unsigned char *mask;
    const float *pre_trans, *gt_trans;
    float *flow, *score;
    unsigned char *mask8;
    float *trans_pred, *trans_gt;
    unsigned char *done;
};

// One workgroup per (chunk of PACK_CHUNK positions, slot); lane t holds position i = p0 + t of the slot and, when i is a valid row of
// the slot's frame, writes packed row off1[f] + i -- flow, score and mask byte -- and nobody else of this slot does.  Positions from
// the count on (the padded part of the batch) are neither read nor written.
__global__ __launch_bounds__(PACK_CHUNK) void pack_results_kernel(const PackArgs a)
{
    const int slot = blockIdx.y, t = threadIdx.x;
    const int i = blockIdx.x * PACK_CHUNK + t;
    const int f = min(max(a.frames[slot], 0), a.F - 1);                    // a bad id lands in a wrong frame, not outside the store
    const long long start = a.off1[f];
    const int room = a.off1[f + 1] - a.off1[f];
    const int cnt = max(0, min(min(a.n1[slot], room), a.N));
    if (start < 0 || start + cnt > a.total) return;                        // offsets that do not describe the store: nothing is written
    if (i < cnt) {
        const size_t src = (size_t)slot * a.N + i, dst = (size_t)start + i;
        const float *s = a.sf + (size_t)slot * 3 * a.N + i;
        a.flow[3 * dst] = s[0];
        a.flow[3 * dst + 1] = s[a.N];
        a.flow[3 * dst + 2] = s[2 * (size_t)a.N];
        if (a.stat_cls) a.score[dst] = a.stat_cls[src];
        a.mask8[dst] = a.mask[src];
    }
    if (blockIdx.x == 0) {
        if (t < 16) {
            a.trans_pred[(size_t)f * 16 + t] = a.pre_trans[(size_t)slot * 16 + t];
            a.trans_gt[(size_t)f * 16 + t] = a.gt_trans[(size_t)slot * 16 + t];
        }
        if (t == 0) a.done[f] = 1;
    }
}

// One lane per clip, its frames in order: P = I; P = P . inv(T_k); poses[k] = P.  inv is the rigid inverse (R^T, -R^T t) whether or
// not R is orthonormal (odometry_util.se3_inverse).  All in float64; a dot product is ((a0 b0 + a1 b1) + a2 b2) + a3 b3 with the
// inverse's bottom row (0, 0, 0, 1) taking part as numbers, and the translation of the inverse is -((r0 t0 + r1 t1) + r2 t2).
__global__ __launch_bounds__(64) void pose_chain_kernel(int F, int C, const float *__restrict__ T, const int *__restrict__ clips,
                                                        double *__restrict__ poses)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const int first = max(clips[2 * c], 0), last = min(clips[2 * c + 1], F);
    double P[3][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}};
    for (int k = first; k < last; ++k) {
        const float *q = T + (size_t)k * 16;
        double M[4][4];
        for (int r = 0; r < 3; ++r) {
            for (int j = 0; j < 3; ++j) M[r][j] = (double)q[4 * j + r];
            M[r][3] = -(((double)q[r] * (double)q[3] + (double)q[4 + r] * (double)q[7]) + (double)q[8 + r] * (double)q[11]);
        }
        M[3][0] = 0.0; M[3][1] = 0.0; M[3][2] = 0.0; M[3][3] = 1.0;
        double Q[3][4];
        for (int r = 0; r < 3; ++r)
            for (int j = 0; j < 4; ++j)
                Q[r][j] = ((P[r][0] * M[0][j] + P[r][1] * M[1][j]) + P[r][2] * M[2][j]) + P[r][3] * M[3][j];
        double *out = poses + (size_t)k * 16;
        for (int r = 0; r < 3; ++r)
            for (int j = 0; j < 4; ++j) {
                P[r][j] = Q[r][j];
                out[4 * r + j] = Q[r][j];
            }
        out[12] = 0.0; out[13] = 0.0; out[14] = 0.0; out[15] = 1.0;
    }
}

}  // namespace

extern "C" int cmf_pack_results(int B, int nmax, int nframes, const int *frames, const int *n1, const int *off1, long long total,
                                const float *sf, const float *stat_cls, const unsigned char *mask, const float *pre_trans,
                                const float *gt_trans, float *flow, float *score, unsigned char *mask8, float *trans_pred,
                                float *trans_gt, unsigned char *done, void *stream)
{
    CMF_CHECK_ARG(B >= 1 && B <= 65535 && nframes >= 1 && total >= 0);     // B is the grid's y extent
    CMF_CHECK_ARG(nmax >= 1 && nmax <= CMF_DRAW_MAX_NPOINTS);
    CMF_CHECK_ARG(frames && n1 && off1 && sf && mask && pre_trans && gt_trans);
    CMF_CHECK_ARG(flow && mask8 && trans_pred && trans_gt && done && (score || !stat_cls));
    PackArgs a{B, nmax, nframes, total, frames, n1, off1, sf, stat_cls, mask, pre_trans, gt_trans, flow, score, mask8, trans_pred, trans_gt, done};
    hipLaunchKernelGGL(pack_results_kernel, dim3(cmf_divup(nmax, PACK_CHUNK), B), dim3(PACK_CHUNK), 0, (hipStream_t)stream, a);
    return cmf_launch_status();
}

extern "C" int cmf_pose_chain(int nframes, int nclips, const float *T, const int *clips, double *poses, void *stream)
{
    CMF_CHECK_ARG(nframes >= 0 && nclips >= 0);
    if (nframes == 0 || nclips == 0) return 0;
    CMF_CHECK_ARG(T && clips && poses);
    hipLaunchKernelGGL(pose_chain_kernel, dim3(cmf_divup(nclips, 64)), dim3(64), 0, (hipStream_t)stream, nframes, nclips, T, clips, poses);
    return cmf_launch_status();
}
