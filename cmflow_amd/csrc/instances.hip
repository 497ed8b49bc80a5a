// Moving-object instances of a test run (cmflow_amd/instances.py): density-based clustering of every selected
// frame's moving points by position and by the displacement they show against the ego-motion.  A DEFINITION, stated in
// include/cmflow_hip.h and restated in numpy, bit for bit, by tests/instances_ref.py: float64 from the float32 inputs, a fixed
// operation order, no contraction anywhere in this file, and no dependence on the order in which threads run.
#include "frame_tables.h"

#pragma clang fp contract(off)

namespace {

constexpr int INST_THREADS = CMF_INST_MAX_POINTS, INST_WAVES = INST_THREADS / CMF_WAVE;      // one thread per candidate slot
constexpr unsigned char KIND_NONE = 0, KIND_NOISE = 1, KIND_BORDER = 2, KIND_CORE = 3;

struct InstArgs {
    int nsel, F, ld_tab, gt, min_points;
    long long total;
    double eps2, w2;
    const long long *frames;
    const int *off1;
    const float *tab1, *flow, *T;
    const unsigned char *mask;
    int *label, *count, *size, *seed;
    unsigned char *kind;
    float *centroid, *disp, *lo, *hi;
};

// One workgroup of 1024 threads per selected frame.  The candidates are compacted into LDS in point order (ft_block_rank of
// frame_tables.h over each chunk of 1024 points), so a candidate's slot c orders like its point index and "lowest index" can be decided
// on slots.  Thread t owns slot t: it alone writes what belongs to it, in LDS and in global memory, and wave w owns the slots
// 64 w .. 64 w + 63 -- a ballot of the wave is word w of a bit set over the slots.
// Every pair distance is formed ONCE: the thread walks all slots j (the same j for every lane: LDS broadcasts) and keeps its row of the
// neighbour relation as 16 words of 64 bits in registers (the word loop is unrolled, so the registers are indexed statically).
// Everything after that walks set bits only.
// Components: Jacobi rounds over two label arrays -- new[i] = old[min(old[i], min over core neighbours j of old[j])] -- with a
// barrier between the rounds, so a round reads only what the previous one wrote and the result of EVERY round, not only the last,
// is independent of the schedule.  Labels are core slots of the point's own component and only decrease; the fixed point is the
// lowest core slot of the component.  The loop ends, for the whole workgroup at once, when a block-wide vote finds no change.
__global__ __launch_bounds__(INST_THREADS) void cluster_moving_kernel(const InstArgs a)
{
    __shared__ double s_d[CMF_INST_MAX_POINTS][3];                         // own-motion displacement of the candidate in slot c
    __shared__ float s_p[CMF_INST_MAX_POINTS][3];
    __shared__ int s_idx[CMF_INST_MAX_POINTS];                             // its frame-local point index
    __shared__ int s_lab[2][CMF_INST_MAX_POINTS];
    __shared__ int s_seed[CMF_INST_MAX_POINTS];                            // slot of instance k's seed
    __shared__ unsigned long long s_core[INST_WAVES];                      // the core slots as a bit set
    __shared__ int s_cnt[INST_WAVES];
    const int tid = threadIdx.x, lane = tid & (CMF_WAVE - 1), wave = tid / CMF_WAVE;
    const int s = blockIdx.x;
    const int f = ft_selected_frame(a.frames, s, a.F);
    long long start, n_ll;
    ft_frame_rows(a.off1, f, a.total, start, n_ll);                        // a frame outside the tables owns no rows
    const int n = (int)n_ll;                                               // total <= INT_MAX
    const size_t row0 = (size_t)start;
    const bool too_large = n > CMF_INST_MAX_POINTS;                        // treated as empty: nothing is a candidate

    // ---- candidates, compacted in point order; everything else is answered at once.  A frame that is not too large is one chunk.
    double T[12];
    for (int e = 0; e < 12; ++e) T[e] = (double)a.T[(size_t)f * 16 + e];
    int m = 0;
    for (int p0 = 0; p0 < n; p0 += INST_THREADS) {                         // n is uniform: every thread passes the same barriers
        const int p = p0 + tid;
        bool cand = false;
        if (p < n) {
            const size_t row = row0 + p;
            cand = !too_large && (a.gt ? a.tab1[row * a.ld_tab + 9] == 0.0f : a.mask[row] == 0);
            if (!cand) {
                a.label[row] = -1;
                a.kind[row] = KIND_NONE;
            }
        }
        int before, all;
        ft_block_rank<INST_WAVES>(cand, lane, wave, s_cnt, before, all);
        if (cand) {                                                        // only where n <= 1024: m + before < n
            const int c = m + before;
            const size_t row = row0 + p;
            const float *q = a.tab1 + row * a.ld_tab;
            const float *fl = a.gt ? q + 6 : a.flow + 3 * row;
            const double px = (double)q[0], py = (double)q[1], pz = (double)q[2];
            s_p[c][0] = q[0]; s_p[c][1] = q[1]; s_p[c][2] = q[2];
            ft_own_motion(T, px, py, pz, fl, s_d[c]);
            s_idx[c] = p;
        }
        m += all;
    }
    __syncthreads();

    // ---- the slot this thread owns, in registers; D2(own, slot j) is the header's expression
    const bool own = tid < m;
    const int me = own ? tid : 0;
    const double px = (double)s_p[me][0], py = (double)s_p[me][1], pz = (double)s_p[me][2];
    const double dx = s_d[me][0], dy = s_d[me][1], dz = s_d[me][2];
    auto d2_to = [&](int j) {
        const double qx = (double)s_p[j][0], qy = (double)s_p[j][1], qz = (double)s_p[j][2];
        const double ex = s_d[j][0], ey = s_d[j][1], ez = s_d[j][2];
        return (((px - qx) * (px - qx) + (py - qy) * (py - qy)) + (pz - qz) * (pz - qz))
               + a.w2 * (((dx - ex) * (dx - ex) + (dy - ey) * (dy - ey)) + (dz - ez) * (dz - ez));
    };

    // ---- the neighbour relation, row by row, and the core test.  A wave without a slot below m skips the walk (uniform).
    unsigned long long nb[INST_WAVES];
    int cnt = 0;
#pragma unroll
    for (int w = 0; w < INST_WAVES; ++w) {
        unsigned long long bits = 0;
        if (wave * CMF_WAVE < m)
            for (int j = w * CMF_WAVE; j < min(m, (w + 1) * CMF_WAVE); ++j) bits |= d2_to(j) <= a.eps2 ? 1ull << (j & (CMF_WAVE - 1)) : 0ull;
        nb[w] = own ? bits : 0ull;
        cnt += __popcll(nb[w]);
    }
    const bool core = own && cnt >= a.min_points;
    {
        const unsigned long long hits = __ballot(core);
        if (lane == 0) s_core[wave] = hits;
    }
    s_lab[0][tid] = core ? tid : -1;
    s_lab[1][tid] = core ? tid : -1;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < INST_WAVES; ++w) nb[w] &= s_core[w];               // from here on: the CORE neighbours

    // ---- components of the core points.  After r rounds a label is at most the lowest core slot within r steps, so m rounds suffice;
    //      a chain needs the most of them, and the jump through old[] shortens it to about log2 of its length.
    int cur = 0;
    for (int round = 0; round < m; ++round) {                              // m and the vote are uniform: no thread leaves before a barrier
        const int *old = s_lab[cur];
        int changed = 0;
        if (core) {
            int best = old[tid];
#pragma unroll
            for (int w = 0; w < INST_WAVES; ++w)
                for (unsigned long long bits = nb[w]; bits; bits &= bits - 1) best = min(best, old[w * CMF_WAVE + __builtin_ctzll(bits)]);
            const int to = old[best];                                      // <= best: a core slot of the same component
            changed = to != old[tid];
            s_lab[cur ^ 1][tid] = to;
        }
        cur ^= 1;
        if (!__syncthreads_or(changed)) break;                             // also the barrier between two rounds
    }
    int *lab = s_lab[cur], *rank = s_lab[cur ^ 1];

    // ---- borders: the core neighbour with the smallest D2, the lowest slot among equals (j ascends, the compare is strict; the
    //      distance is the one the neighbour test saw, formed again from the same operands).  Only the owner touches a non-core
    //      slot of lab, and core slots are not written here.
    unsigned char kind = core ? KIND_CORE : KIND_NOISE;
    if (own && !core) {
        int to = -1;
        double d2min = 0.0;
#pragma unroll
        for (int w = 0; w < INST_WAVES; ++w)
            for (unsigned long long bits = nb[w]; bits; bits &= bits - 1) {
                const int j = w * CMF_WAVE + __builtin_ctzll(bits);
                const double d2 = d2_to(j);
                if (to < 0 || d2 < d2min) {
                    to = j;
                    d2min = d2;
                }
            }
        if (to >= 0) {
            kind = KIND_BORDER;
            lab[tid] = lab[to];
        }
    }
    __syncthreads();

    // ---- numbering: the seeds (core slots that carry their own label) in ascending order
    int K;
    {
        const bool root = core && lab[tid] == tid;
        int before;
        ft_block_rank<INST_WAVES>(root, lane, wave, s_cnt, before, K);
        if (root) {
            rank[tid] = before;
            s_seed[before] = tid;
        }
    }
    __syncthreads();
    // the instance id of every slot, written out and kept in place: a slot of lab is read and written by its owner only, rank is
    // read by everybody and written by nobody
    if (own) {
        const int id = lab[tid] >= 0 ? rank[lab[tid]] : -1;                // lab[tid] is a seed or -1, rank is written at the seeds
        const size_t row = row0 + s_idx[tid];
        a.label[row] = id;
        a.kind[row] = kind;
        lab[tid] = id;
    }
    __syncthreads();

    // ---- statistics: one thread per instance, its members in ascending point order, sums from 0.0
    if (tid == 0) a.count[f] = K;
    for (int k = tid; k < n; k += INST_THREADS) {
        const size_t row = row0 + k;
        int size = 0;
        double S[3] = {0.0, 0.0, 0.0}, E[3] = {0.0, 0.0, 0.0};
        float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f};
        if (k < K) {
            for (int c = 0; c < m; ++c) {
                if (lab[c] != k) continue;
                for (int r = 0; r < 3; ++r) {
                    const float v = s_p[c][r];
                    S[r] = S[r] + (double)v;
                    E[r] = E[r] + s_d[c][r];
                    if (size == 0 || v < lo[r]) lo[r] = v;
                    if (size == 0 || v > hi[r]) hi[r] = v;
                }
                ++size;
            }
        }
        a.size[row] = size;
        a.seed[row] = k < K ? s_idx[s_seed[k]] : -1;
        for (int r = 0; r < 3; ++r) {
            a.centroid[3 * row + r] = k < K ? (float)(S[r] / (double)size) : 0.0f;
            a.disp[3 * row + r] = k < K ? (float)(E[r] / (double)size) : 0.0f;
            a.lo[3 * row + r] = lo[r];
            a.hi[3 * row + r] = hi[r];
        }
    }
}

}  // namespace

extern "C" int cmf_cluster_moving(int nsel, int nframes, const long long *frames, const int *off1, long long total, const float *tab1,
                                  int ld_tab, const float *flow, const unsigned char *mask, const float *T, int gt, double eps2,
                                  double w2, int min_points, int *label, unsigned char *kind, int *count, int *size, int *seed,
                                  float *centroid, float *disp, float *lo, float *hi, void *stream)
{
    CMF_CHECK_ARG(nsel >= 0 && nframes >= 1 && total >= 0 && total <= 2147483647LL && min_points >= 1);
    CMF_CHECK_ARG(eps2 == eps2 && w2 == w2);
    if (nsel == 0) return 0;
    CMF_CHECK_ARG(frames || nsel <= nframes);
    CMF_CHECK_ARG(off1 && tab1 && ld_tab >= 10 && T && count);
    CMF_CHECK_ARG(gt || (mask && flow));
    CMF_CHECK_ARG(total == 0 || (label && kind && size && seed && centroid && disp && lo && hi));
    InstArgs a{nsel, nframes, ld_tab, gt ? 1 : 0, min_points, total, eps2, w2, frames, off1, tab1, flow, T, mask,
               label, count, size, seed, kind, centroid, disp, lo, hi};
    hipLaunchKernelGGL(cluster_moving_kernel, dim3(nsel), dim3(INST_THREADS), 0, (hipStream_t)stream, a);
    return cmf_launch_status();
}
