// A test run's clouds accumulated over a window of frames (cmflow_amd/accumulate.py): the last W scans of a clip
// brought into the current sensor frame -- static points through the chained ego-motion, moving points left as a trail, dropped, or
// carried forward by their own flow.  A DEFINITION, stated in include/cmflow_hip.h and restated in numpy, bit for bit, by
// tests/accumulate_ref.py: float64 from the float32 inputs, a fixed operation order, no contraction anywhere in this file.
#include "frame_tables.h"

#pragma clang fp contract(off)

namespace {

constexpr int ACC_THREADS = 256, ACC_WAVES = ACC_THREADS / CMF_WAVE;

struct AccArgs {
    int nsel, F, ld_tab, window, mode, gt;
    long long total, cap_total;
    const long long *frames;
    const int *first, *off1, *cap_off;
    const float *tab1, *flow, *T;
    const unsigned char *mask;
    float *xyz;
    int *src, *count;
    unsigned char *age;
};

// One workgroup per target.  The transforms of the window pass through LDS (one coalesced read), lane 0 forms the chain M_0 .. M_G-1
// from them in order (a parallel scan would change the association), and the ages are then walked oldest first with a running row
// offset: thread t takes point c * 256 + t of the source frame and writes output row base + (its rank among the kept points), so a
// target's rows keep age order and, inside an age, the frame's own point order.  Nothing but `drop` leaves a point out, and only `drop`
// needs the ranks (ft_block_rank of frame_tables.h).  Rows from the count to the capacity are
// written as padding by the same workgroup, so every row of the capacity is written exactly once.
template <bool DROP>
__global__ __launch_bounds__(ACC_THREADS) void accumulate_kernel(const AccArgs a)
{
    __shared__ double s_M[CMF_ACCUM_MAX_WINDOW][12];
    __shared__ float s_T[CMF_ACCUM_MAX_WINDOW][12];                        // s_T[g] = the first three rows of T_{j-g}, g >= 1
    __shared__ int s_cnt[ACC_WAVES];
    const int tid = threadIdx.x, lane = tid & (CMF_WAVE - 1), wave = tid / CMF_WAVE;
    const int s = blockIdx.x;
    const int j = ft_selected_frame(a.frames, s, a.F);
    const int first = min(max(a.first[s], 0), j);
    const int G = min(a.window, j - first + 1);                            // 1 <= G <= CMF_ACCUM_MAX_WINDOW: sources j-G+1 .. j, all >= first >= 0
    const long long cap0 = a.cap_off[s];
    long long cap = (long long)a.cap_off[s + 1] - cap0;
    if (cap0 < 0 || cap < 0 || cap0 + cap > a.cap_total) cap = 0;          // offsets that do not describe the outputs: nothing is written

    for (int k = tid; k < (G - 1) * 12; k += ACC_THREADS) {
        const int g = k / 12 + 1;
        s_T[g][k % 12] = a.T[(size_t)(j - g) * 16 + k % 12];
    }
    __syncthreads();
    if (tid == 0) {
        double M[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
        for (int e = 0; e < 12; ++e) s_M[0][e] = M[e];
        for (int g = 1; g < G; ++g) {
            double t[12], Q[12];
            for (int e = 0; e < 12; ++e) t[e] = (double)s_T[g][e];
            for (int r = 0; r < 3; ++r) {
                const double *m = M + 4 * r;
                for (int c = 0; c < 3; ++c) Q[4 * r + c] = (m[0] * t[c] + m[1] * t[4 + c]) + m[2] * t[8 + c];
                Q[4 * r + 3] = ((m[0] * t[3] + m[1] * t[7]) + m[2] * t[11]) + m[3];
            }
            for (int e = 0; e < 12; ++e) {
                M[e] = Q[e];
                s_M[g][e] = Q[e];
            }
        }
    }
    __syncthreads();

    long long base = 0;                                                    // rows of this target written so far
    for (int g = G - 1; g >= 0; --g) {
        const int i = j - g;
        long long start, n;
        ft_frame_rows(a.off1, i, a.total, start, n);                       // a frame outside the tables is empty
        const double *M = s_M[g], *N = s_M[g > 0 ? g - 1 : 0];
        const float *Ti = s_T[g];
        for (long long p0 = 0; p0 < n; p0 += ACC_THREADS) {
            const long long p = p0 + tid;
            bool keep = false, moving = false;
            size_t row = 0;
            if (p < n) {
                row = (size_t)(start + p);
                moving = a.gt ? a.tab1[row * a.ld_tab + 9] == 0.0f : a.mask[row] == 0;
                keep = !(DROP && moving && g > 0);
            }
            long long dst = base + (p - p0);
            if (DROP) {
                int before, all;
                ft_block_rank<ACC_WAVES>(keep, lane, wave, s_cnt, before, all);
                dst = base + before;
                base += all;
            } else {
                base += min((long long)ACC_THREADS, n - p0);
            }
            if (keep && dst < cap) {
                const float *q = a.tab1 + row * a.ld_tab;
                float *o = a.xyz + 3 * (size_t)(cap0 + dst);
                if (g == 0) {
                    o[0] = q[0]; o[1] = q[1]; o[2] = q[2];                 // the current scan: copied bit for bit
                } else {
                    const double px = (double)q[0], py = (double)q[1], pz = (double)q[2];
                    double x = ft_affine(M, px, py, pz), y = ft_affine(M + 4, px, py, pz), z = ft_affine(M + 8, px, py, pz);
                    if (a.mode == CMF_ACCUM_PROPAGATE && moving) {
                        const float *f = a.gt ? q + 6 : a.flow + 3 * row;
                        double t[12], d[3];
                        for (int e = 0; e < 12; ++e) t[e] = (double)Ti[e];
                        ft_own_motion(t, px, py, pz, f, d);
                        const double k = (double)g;
                        x = x + k * ((N[0] * d[0] + N[1] * d[1]) + N[2] * d[2]);
                        y = y + k * ((N[4] * d[0] + N[5] * d[1]) + N[6] * d[2]);
                        z = z + k * ((N[8] * d[0] + N[9] * d[1]) + N[10] * d[2]);
                    }
                    o[0] = (float)x; o[1] = (float)y; o[2] = (float)z;
                }
                a.src[cap0 + dst] = (int)row;
                a.age[cap0 + dst] = (unsigned char)g;
            }
        }
    }
    const long long cnt = base < cap ? base : cap;
    if (tid == 0) a.count[s] = (int)cnt;
    for (long long r = cnt + tid; r < cap; r += ACC_THREADS) {             // behind the count: xyz 0, src -1, age 255
        float *o = a.xyz + 3 * (size_t)(cap0 + r);
        o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f;
        a.src[cap0 + r] = -1;
        a.age[cap0 + r] = 255;
    }
}

}  // namespace

extern "C" int cmf_accumulate(int nsel, int nframes, const long long *frames, const int *first, const int *off1, long long total,
                              const float *tab1, int ld_tab, const float *flow, const unsigned char *mask, const float *T, int window,
                              int mode, int gt, const int *cap_off, long long cap_total, float *xyz, int *src, unsigned char *age,
                              int *count, void *stream)
{
    CMF_CHECK_ARG(nsel >= 0 && nframes >= 1 && total >= 0 && total <= 2147483647LL && cap_total >= 0 && cap_total <= 2147483647LL);
    CMF_CHECK_ARG(window >= 1 && window <= CMF_ACCUM_MAX_WINDOW && mode >= CMF_ACCUM_KEEP && mode <= CMF_ACCUM_DROP);
    if (nsel == 0) return 0;
    CMF_CHECK_ARG(frames || nsel <= nframes);
    CMF_CHECK_ARG(first && off1 && tab1 && ld_tab >= 10 && T && cap_off && count);
    CMF_CHECK_ARG(gt || mask);
    CMF_CHECK_ARG(gt || mode != CMF_ACCUM_PROPAGATE || flow);
    CMF_CHECK_ARG(cap_total == 0 || (xyz && src && age));
    AccArgs a{nsel, nframes, ld_tab, window, mode, gt ? 1 : 0, total, cap_total, frames, first, off1, cap_off, tab1, flow, T, mask, xyz, src, count, age};
    if (mode == CMF_ACCUM_DROP)
        hipLaunchKernelGGL(accumulate_kernel<true>, dim3(nsel), dim3(ACC_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(accumulate_kernel<false>, dim3(nsel), dim3(ACC_THREADS), 0, (hipStream_t)stream, a);
    return cmf_launch_status();
}
