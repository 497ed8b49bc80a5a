// Moving-object instances tracked across the frames of a clip (cmflow_amd/tracks.py): every frame's instances
// (cmf_cluster_moving's tables) associated with the tracks the earlier frames of the clip left, by a gated greedy nearest-first
// matching against a constant-displacement prediction.  A DEFINITION, stated in include/cmflow_hip.h and restated in numpy, bit for
// bit, by tests/tracks_ref.py: float64 from the float32 inputs, a fixed operation order, no contraction anywhere in this file, and
// no dependence on the order in which threads run.
#include "frame_tables.h"

#pragma clang fp contract(off)

namespace {

constexpr int TRK_THREADS = CMF_TRACK_MAX_LIVE, TRK_WAVES = TRK_THREADS / CMF_WAVE;          // one thread per live slot and per instance

struct TrackArgs {
    int C, F, max_gap;
    long long total;
    double gate2;
    const int *clips, *off1, *count, *label;
    const float *centroid, *disp, *T;
    int *track, *prev_row, *gap, *age, *point_track, *birth, *last, *hits, *ntracks, *overflow;
    float *pred;
};

// G2 of the header: e_r = P_r - c_r, (e0 e0 + e1 e1) + e2 e2 -- ONE expression for both sides of an edge, so a cost formed again
// (by the track, by the instance, in a later round) is formed from the same operands in the same order
__device__ __forceinline__ double trk_g2(double p0, double p1, double p2, const float *c)
{
    const double e0 = p0 - (double)c[0], e1 = p1 - (double)c[1], e2 = p2 - (double)c[2];
    return (e0 * e0 + e1 * e1) + e2 * e2;
}

// One workgroup of 1024 threads per clip, the clip's frames in sequence.  Thread t owns live SLOT t -- a track keeps its slot from
// birth to death, its state (P, D, the counters) stays in the owner's registers, and only what other threads read is published to
// LDS each frame (P and the track id) -- and INSTANCE t of the current frame.  The live list "in ascending track id" of the
// definition is the set of live slots with their ids: wherever the order matters (the tie between two tracks equally far from an
// instance) the ids are compared, so the slot a track sits in never shows in a result.  A birth takes the lowest free slot (a ballot
// scan over the free slots against a ballot scan over the unmatched instances), which keeps the live slots below a low high-water
// mark.
// Association: mutual-best rounds over what is still unmatched, kept as two bit sets in LDS (free slots, free instances; a wave's
// ballot is one word).  A track walks the free instances and picks its best edge by (G2, j), an instance walks the free slots and
// picks its best edge by (G2, track id) -- the same address for every lane, LDS broadcasts; both picks go to LDS, a barrier, and
// pairs that picked each other match.  Both orders are restrictions of the one total order (G2, track id, j), so the smallest
// remaining edge is always mutual and the fixed point is the sorted greedy matching of the definition.  Nothing is kept between
// the rounds but the sets: a cost is formed again from the same operands by the same expression.  A round reads only what the
// round before wrote (the picks and the sets, a barrier on either side), so every round's outcome, not only the last, is
// independent of the schedule.  The loop ends for the whole workgroup at once when a block-wide vote finds no new pair, after
// min(live, K) rounds at the most.  A round costs a thread the free slots plus the free instances; a frame whose tracks all find
// their instance at once takes two rounds, and only a chain of displaced choices (the ladder of the tests) takes one round per pair.
// Every barrier is passed by every thread: the clip's bounds, a frame's validity, n, K and the round count are uniform.
__global__ __launch_bounds__(TRK_THREADS) void track_instances_kernel(const TrackArgs a)
{
    __shared__ double s_P[TRK_THREADS][3];                                 // the predicted position of the track in slot u
    __shared__ float s_c[TRK_THREADS][3], s_d[TRK_THREADS][3];             // the centroid and the displacement of instance j
    __shared__ int s_id[TRK_THREADS];                                      // the track id of slot u
    __shared__ int s_tpick[TRK_THREADS], s_ipick[TRK_THREADS];             // the round's picks: of slot u (an instance), of instance j (a slot)
    int *const s_itrack = s_ipick;                                         // after the rounds: the track id instance j got,
    int *const s_born = s_tpick;                                           //   the instance that opens the r-th new track of the frame
    __shared__ unsigned long long s_tfree[TRK_WAVES], s_ifree[TRK_WAVES];  // bit sets: the live slots, the instances, not matched yet
    __shared__ int s_cnt[TRK_WAVES];
    const int tid = threadIdx.x, lane = tid & (CMF_WAVE - 1), wave = tid / CMF_WAVE;
    const int clip = blockIdx.x;
    // ft_clip and, per frame, ft_clip_frame / ft_clip_frame_instances of frame_tables.h, written out: this kernel's inner loops are
    // scheduled differently around the inlined helpers and the launch takes 1 % longer
    int first = a.clips[2 * clip], end = a.clips[2 * clip + 1];
    first = first < 0 ? 0 : first > a.F ? a.F : first;
    end = end < first ? first : end > a.F ? a.F : end;
    const long long base = a.off1[first];
    const bool clip_ok = base >= 0 && base <= a.total;                     // a clip that starts outside the tables owns no rows

    // ---- the slot's state
    bool live = false;
    double P0 = 0.0, P1 = 0.0, P2 = 0.0, D0 = 0.0, D1 = 0.0, D2 = 0.0;
    int id = -1, miss = 0, hits = 0, last_row = -1, born_f = -1, last_f = -1;
    int next_id = 0, overflow = 0;                                         // uniform
    long long top = base;                                                  // the end of the clip's last frame that owns rows

    auto close_track = [&]() {                                             // the track's row of the per-track tables: base + id < top
        const size_t row = (size_t)base + id;
        a.birth[row] = born_f;
        a.last[row] = last_f;
        a.hits[row] = hits;
    };

    for (int f = first; f < end; ++f) {
        const long long start = a.off1[f], stop = a.off1[f + 1];
        const bool owns = clip_ok && start >= top && stop >= start && stop <= a.total;    // in order inside the tables: the frames' rows are disjoint
        const int n = owns ? (int)(stop - start) : 0;
        if (owns) top = stop;
        const size_t row0 = owns ? (size_t)start : 0;
        int K = owns ? a.count[f] : 0;
        K = K < 0 ? 0 : K > n ? n : K;
        K = K > CMF_TRACK_MAX_LIVE ? CMF_TRACK_MAX_LIVE : K;
        float Tf[12];                                                      // uniform, asked for before anything waits
        for (int e = 0; e < 12; ++e) Tf[e] = a.T[(size_t)f * 16 + e];

        // ---- publish: the tracks' predictions and ids, the frame's centroids
        const bool isI = tid < K;
        if (live) {
            s_P[tid][0] = P0; s_P[tid][1] = P1; s_P[tid][2] = P2;
            s_id[tid] = id;
        }
        if (isI)
            for (int r = 0; r < 3; ++r) {
                s_c[tid][r] = a.centroid[3 * (row0 + tid) + r];
                s_d[tid][r] = a.disp[3 * (row0 + tid) + r];
            }
        {
            const unsigned long long alive = __ballot(live), inst = __ballot(isI);
            if (lane == 0) {
                s_tfree[wave] = alive;
                s_ifree[wave] = inst;
            }
        }
        __syncthreads();
        int L = 0;                                                         // the live tracks
        for (int w = 0; w < TRK_WAVES; ++w) L += __popcll(s_tfree[w]);
        const float *mine = s_c[isI ? tid : 0];

        // ---- mutual-best rounds
        int mj = -1, mu = -1;                                              // the instance this slot's track matched, the slot this instance matched
        const int rounds = min(L, K);
        for (int round = 0; round < rounds; ++round) {
            int tp = -1, ip = -1;
            if (live && mj < 0) {
                double best = 0.0;
                for (int w = 0; w < TRK_WAVES; ++w)
                    for (unsigned long long bits = s_ifree[w]; bits; bits &= bits - 1) {
                        const int j = w * CMF_WAVE + __builtin_ctzll(bits);                  // ascending, a strict compare: the lowest j among equals
                        const double g = trk_g2(P0, P1, P2, s_c[j]);
                        if (g <= a.gate2 && (tp < 0 || g < best)) {
                            tp = j;
                            best = g;
                        }
                    }
            }
            if (isI && mu < 0) {
                double best = 0.0;
                int best_id = 0;
                for (int w = 0; w < TRK_WAVES; ++w)
                    for (unsigned long long bits = s_tfree[w]; bits; bits &= bits - 1) {
                        const int u = w * CMF_WAVE + __builtin_ctzll(bits);
                        const double g = trk_g2(s_P[u][0], s_P[u][1], s_P[u][2], mine);
                        const int uid = s_id[u];
                        if (g <= a.gate2 && (ip < 0 || g < best || (g == best && uid < best_id))) {   // the lowest track id among equals
                            ip = u;
                            best = g;
                            best_id = uid;
                        }
                    }
            }
            s_tpick[tid] = tp;
            s_ipick[tid] = ip;
            __syncthreads();
            const bool t_now = tp >= 0 && s_ipick[tp] == tid, i_now = ip >= 0 && s_tpick[ip] == tid;
            if (t_now) mj = tp;
            if (i_now) mu = ip;
            const unsigned long long bt = __ballot(t_now), bi = __ballot(i_now);
            if (lane == 0) {
                s_tfree[wave] &= ~bt;
                s_ifree[wave] &= ~bi;
            }
            if (!__syncthreads_or(t_now)) break;                           // also the barrier between two rounds
        }

        // ---- matched: the track's owner writes its instance's row, then takes the measurement
        bool coasting = false, dying = false;
        if (live) {
            if (mj >= 0) {
                const size_t row = row0 + mj;
                hits += 1;
                a.track[row] = id;
                a.prev_row[row] = last_row;
                a.gap[row] = f - last_f;
                a.age[row] = hits;
                a.pred[3 * row + 0] = (float)P0; a.pred[3 * row + 1] = (float)P1; a.pred[3 * row + 2] = (float)P2;
                s_itrack[mj] = id;
                P0 = (double)s_c[mj][0]; P1 = (double)s_c[mj][1]; P2 = (double)s_c[mj][2];
                D0 = (double)s_d[mj][0]; D1 = (double)s_d[mj][1]; D2 = (double)s_d[mj][2];
                miss = 0;
                last_row = (int)row;
                last_f = f;
            } else {
                miss += 1;
                dying = miss > a.max_gap;
                coasting = !dying;
            }
        }
        // ---- unmatched instances open tracks, in ascending j: the instance's owner writes its row
        const bool born = isI && mu < 0;
        int r_born, births, r_coast, coasts;
        ft_block_rank<TRK_WAVES>(born, lane, wave, s_cnt, r_born, births);
        if (born) {
            const size_t row = row0 + tid;
            a.track[row] = next_id + r_born;
            a.prev_row[row] = -1;
            a.gap[row] = 0;
            a.age[row] = 1;
            for (int r = 0; r < 3; ++r) a.pred[3 * row + r] = s_c[tid][r];
            s_itrack[tid] = next_id + r_born;
            s_born[r_born] = tid;
        }
        // ---- capacity: matched tracks and births are K <= 1024 and always fit; the coasting tracks go first
        ft_block_rank<TRK_WAVES>(coasting, lane, wave, s_cnt, r_coast, coasts);
        if (K + coasts > CMF_TRACK_MAX_LIVE) {
            overflow += 1;
            dying = dying || coasting;
            coasting = false;
        }
        if (dying) {
            close_track();
            live = false;
        }
        if (coasting) {                                                    // P stays; D into the axes of the next frame's scan 1
            const double d0 = D0, d1 = D1, d2 = D2;
            D0 = ((double)Tf[0] * d0 + (double)Tf[1] * d1) + (double)Tf[2] * d2;
            D1 = ((double)Tf[4] * d0 + (double)Tf[5] * d1) + (double)Tf[6] * d2;
            D2 = ((double)Tf[8] * d0 + (double)Tf[9] * d1) + (double)Tf[10] * d2;
        }
        // ---- the births take the lowest free slots (the scan's barriers are also what makes s_born and s_itrack visible)
        {
            int r_free, frees;
            ft_block_rank<TRK_WAVES>(!live, lane, wave, s_cnt, r_free, frees);
            if (!live && r_free < births) {                                // survivors + births <= 1024: frees >= births
                const int j = s_born[r_free];
                const size_t row = row0 + j;
                live = true;
                id = next_id + r_free;
                P0 = (double)s_c[j][0]; P1 = (double)s_c[j][1]; P2 = (double)s_c[j][2];
                D0 = (double)s_d[j][0]; D1 = (double)s_d[j][1]; D2 = (double)s_d[j][2];
                miss = 0;
                hits = 1;
                last_row = (int)row;
                born_f = f;
                last_f = f;
            }
        }
        next_id += births;
        // ---- every live track's prediction into the next frame
        if (live) {
            const double p0 = P0, p1 = P1, p2 = P2;
            P0 = ((((double)Tf[0] * p0 + (double)Tf[1] * p1) + (double)Tf[2] * p2) + (double)Tf[3]) + D0;
            P1 = ((((double)Tf[4] * p0 + (double)Tf[5] * p1) + (double)Tf[6] * p2) + (double)Tf[7]) + D1;
            P2 = ((((double)Tf[8] * p0 + (double)Tf[9] * p1) + (double)Tf[10] * p2) + (double)Tf[11]) + D2;
        }
        // ---- the rows behind K, and every point's track
        for (int p = tid; p < n; p += TRK_THREADS) {
            const size_t row = row0 + p;
            if (p >= K) {
                a.track[row] = -1;
                a.prev_row[row] = -1;
                a.gap[row] = 0;
                a.age[row] = 0;
                for (int r = 0; r < 3; ++r) a.pred[3 * row + r] = 0.0f;
            }
            const int l = a.label[row];
            a.point_track[row] = l >= 0 && l < K ? s_itrack[l] : -1;
        }
        __syncthreads();                                                   // the next frame overwrites what this one published
    }

    // ---- the clip's end: the tracks still alive, the counts, and the rows of the per-track tables behind the last track
    if (live) close_track();
    if (tid == 0) {
        a.ntracks[clip] = next_id;
        a.overflow[clip] = overflow;
    }
    top = base;
    for (int f = first; f < end; ++f) {
        const long long start = a.off1[f], stop = a.off1[f + 1];
        if (!(clip_ok && start >= top && stop >= start && stop <= a.total)) continue;       // uniform
        top = stop;
        for (long long row = start + tid; row < stop; row += TRK_THREADS)
            if (row >= base + next_id) {
                a.birth[row] = -1;
                a.last[row] = -1;
                a.hits[row] = 0;
            }
    }
}

}  // namespace

extern "C" int cmf_track_instances(int nclips, int nframes, const int *clips, const int *off1, long long total, const int *count,
                                   const int *label, const float *centroid, const float *disp, const float *T, double gate2,
                                   int max_gap, int *track, int *prev_row, int *gap, int *age, float *pred, int *point_track,
                                   int *birth, int *last, int *hits, int *ntracks, int *overflow, void *stream)
{
    CMF_CHECK_ARG(nclips >= 0 && nframes >= 1 && total >= 0 && total <= 2147483647LL);
    CMF_CHECK_ARG(gate2 == gate2 && max_gap >= 0 && max_gap <= CMF_TRACK_MAX_GAP);
    if (nclips == 0) return 0;
    CMF_CHECK_ARG(clips && off1 && count && T && ntracks && overflow);
    CMF_CHECK_ARG(total == 0 || (label && centroid && disp && track && prev_row && gap && age && pred && point_track && birth && last && hits));
    TrackArgs a{nclips, nframes, max_gap, total, gate2, clips, off1, count, label, centroid, disp, T,
                track, prev_row, gap, age, point_track, birth, last, hits, ntracks, overflow, pred};
    hipLaunchKernelGGL(track_instances_kernel, dim3(nclips), dim3(TRK_THREADS), 0, (hipStream_t)stream, a);
    return cmf_launch_status();
}
