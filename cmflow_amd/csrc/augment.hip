// cmf_augment_batch: one label-consistent transform per slot of a drawn batch, in place (cmflow_amd/dataset.py augment_batch;
// DESIGN.md section 19) -- a rotation about the sensor's z axis after an optional mirror of the y axis, applied to the clouds, the
// flow labels and gt_trans, with the slot's radar-to-camera transform written next to them.  The rule -- generator, angle, operation
// order -- is the one of include/cmflow_hip.h; tests/augment_ref.py restates it in numpy, bit for bit, so nothing here may be
// contracted or reassociated.  One workgroup per (chunk of AUG_CHUNK positions, slot); lane t holds position p0 + t, so every load
// and store runs over consecutive addresses of its tensor, as in draw_frames_kernel.
#include "cmf_common.h"
#include "philox.h"
#include "../../include/cmflow_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int AUG_CHUNK = 256;

struct AugArgs {
    int B, n1, n2, slot0, mirror;
    uint32_t k0, k1;
    double tan_half_max;
    const float *t_cr;
    float *pc1, *pc2, *flow_label, *gt_trans, *aug, *calib;
};

// (a0 b0 + a1 b1) + a2 b2 in float64, every operation rounded on its own
__device__ inline double aug_dot3(double a0, double b0, double a1, double b1, double a2, double b2)
{
    return __dadd_rn(__dadd_rn(__dmul_rn(a0, b0), __dmul_rn(a1, b1)), __dmul_rn(a2, b2));
}

// gt_trans, aug and calib of one slot (one lane): float64 from the float32 entries of A, each result rounded to float32 once
__device__ void aug_transforms(const AugArgs &a, int slot, float cf, float sf, float m, bool identity)
{
    float *G = a.gt_trans + (size_t)slot * 16, *U = a.aug + (size_t)slot * 16, *C = a.calib + (size_t)slot * 16;
    const float Af[3][3] = {{cf, -(m * sf), 0.f}, {sf, m * cf, 0.f}, {0.f, 0.f, 1.f}};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) U[4 * i + j] = identity ? (i == j ? 1.f : 0.f) : Af[i][j];
        U[4 * i + 3] = 0.f;
    }
    if (identity) {
        for (int e = 0; e < 12; ++e) C[e] = a.t_cr[e];
    } else {
        double A[3][3], R[3][3], t[3], H[3][3];
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) { A[i][j] = (double)Af[i][j]; R[i][j] = (double)G[4 * i + j]; }
            t[i] = (double)G[4 * i + 3];
        }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) H[i][j] = aug_dot3(R[i][0], A[j][0], R[i][1], A[j][1], R[i][2], A[j][2]);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) {
                G[4 * i + j] = (float)aug_dot3(A[i][0], H[0][j], A[i][1], H[1][j], A[i][2], H[2][j]);
                C[4 * i + j] = (float)aug_dot3((double)a.t_cr[4 * i], A[j][0], (double)a.t_cr[4 * i + 1], A[j][1],
                                               (double)a.t_cr[4 * i + 2], A[j][2]);
            }
            G[4 * i + 3] = (float)aug_dot3(A[i][0], t[0], A[i][1], t[1], A[i][2], t[2]);
            C[4 * i + 3] = a.t_cr[4 * i + 3];
        }
        G[12] = 0.f; G[13] = 0.f; G[14] = 0.f; G[15] = 1.f;
    }
    for (int e = 12; e < 16; ++e) { U[e] = e == 15 ? 1.f : 0.f; C[e] = e == 15 ? 1.f : 0.f; }
}

__global__ __launch_bounds__(AUG_CHUNK) void augment_batch_kernel(const AugArgs a)
{
    __shared__ float sA[3];                                                // cf, sf, m of the slot
    const int chunk = blockIdx.x, slot = blockIdx.y, t = threadIdx.x;
    if (t == 0) {
        const Philox w = philox4x32_10((uint32_t)(a.slot0 + slot), 2u, 0u, 0u, a.k0, a.k1);
        const double r = __dmul_rn((double)w.x, 0x1p-32);
        const double tn = __dmul_rn(__dsub_rn(__dmul_rn(2.0, r), 1.0), a.tan_half_max);
        const double q = __dmul_rn(tn, tn), d = __dadd_rn(1.0, q);
        const float cf = (float)__ddiv_rn(__dsub_rn(1.0, q), d), sf = (float)__ddiv_rn(__dmul_rn(2.0, tn), d);
        const float m = (a.mirror && (w.y >> 31)) ? -1.f : 1.f;
        sA[0] = cf; sA[1] = sf; sA[2] = m;
        if (chunk == 0) aug_transforms(a, slot, cf, sf, m, cf == 1.f && sf == 0.f && m == 1.f);
    }
    __syncthreads();
    const float cf = sA[0], sf = sA[1], m = sA[2];
    if (cf == 1.f && sf == 0.f && m == 1.f) return;                        // the exact identity: nothing is rewritten (whole workgroup)
    const int p0 = chunk * AUG_CHUNK, p = p0 + t;
    const int N[2] = {a.n1, a.n2};
    float *pc[2] = {a.pc1, a.pc2};
#pragma unroll
    for (int cloud = 0; cloud < 2; ++cloud)                                // (B,3,N): rows x and y of the slot, z stays
        if (p < N[cloud]) {
            float *px = pc[cloud] + (size_t)slot * 3 * N[cloud] + p, *py = px + N[cloud];
            const float x = *px, ym = __fmul_rn(m, *py);
            *px = __fsub_rn(__fmul_rn(cf, x), __fmul_rn(sf, ym));
            *py = __fadd_rn(__fmul_rn(sf, x), __fmul_rn(cf, ym));
        }
    // (B,n1,3): element e of the chunk's 3 * cnt floats belongs to row e / 3; a row's x and y are read by two lanes, possibly of two
    // waves, so every lane forms its value first and the stores follow a barrier
    const int cnt = max(0, min(AUG_CHUNK, a.n1 - p0));
    float *fl = a.flow_label + ((size_t)slot * a.n1 + p0) * 3;
    float v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int e = t + k * AUG_CHUNK;
        v[k] = 0.f;
        if (e < 3 * cnt) {
            const int j = e / 3, c = e - 3 * j;
            if (c < 2) {
                const float x = fl[3 * j], ym = __fmul_rn(m, fl[3 * j + 1]);
                v[k] = c == 0 ? __fsub_rn(__fmul_rn(cf, x), __fmul_rn(sf, ym)) : __fadd_rn(__fmul_rn(sf, x), __fmul_rn(cf, ym));
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int e = t + k * AUG_CHUNK;
        if (e < 3 * cnt && e % 3 < 2) fl[e] = v[k];
    }
}

}  // namespace

extern "C" int cmf_augment_batch(int slot0, int B, int n1, int n2, unsigned long long seed, unsigned long long aug_draw,
                                 double tan_half_max, int mirror, const float *t_camera_radar, float *pc1, float *pc2, float *flow_label,
                                 float *gt_trans, float *aug, float *calib, void *stream)
{
    CMF_CHECK_ARG(slot0 >= 0 && B >= 1 && B <= 65535 && (long long)slot0 + B <= 2147483647LL);     // B is the grid's y extent
    CMF_CHECK_ARG(n1 >= 1 && n1 <= CMF_DRAW_MAX_NPOINTS && n2 >= 1 && n2 <= CMF_DRAW_MAX_NPOINTS);
    CMF_CHECK_ARG(tan_half_max >= 0.0 && tan_half_max <= 1.7976931348623157e308);                  // finite (a NaN fails both)
    CMF_CHECK_ARG(t_camera_radar && pc1 && pc2 && flow_label && gt_trans && aug && calib);
    const Philox key = philox_call_key(seed, aug_draw);
    AugArgs a{B, n1, n2, slot0, mirror, key.x, key.y, tan_half_max, t_camera_radar, pc1, pc2, flow_label, gt_trans, aug, calib};
    hipLaunchKernelGGL(augment_batch_kernel, dim3(cmf_divup(std::max(n1, n2), AUG_CHUNK), B), dim3(AUG_CHUNK), 0, (hipStream_t)stream, a);
    return cmf_launch_status();
}
