// A test run's tracks and objects scored against the labels' (cmflow_amd/score.py): per frame the instances of
// two sides of the chain matched by their point overlap -- both sides partition the SAME points, so an overlap above one half fixes
// the correspondence without an assignment problem -- and per clip the identity walk of MOTS over the gt side's tracks.  A
// DEFINITION, stated in include/cmflow_hip.h and restated in numpy, bit for bit, by tests/score_ref.py: integers everywhere but ONE
// float64 division per candidate pair and its strict compare, no contraction anywhere in this file, and no dependence on the order
// in which threads run.
#include "frame_tables.h"

#pragma clang fp contract(off)

namespace {

constexpr int SCO_THREADS = CMF_INST_MAX_POINTS;                                                // one thread per point and per instance
constexpr int SCO_SHIFT = 11;                                                                   // a label + 1 is 0 .. 1024: eleven bits
static_assert(CMF_INST_MAX_POINTS == CMF_TRACK_MAX_LIVE && CMF_TRACK_MAX_LIVE < (1 << SCO_SHIFT), "one thread per point and per instance");

struct ScoreArgs {
    int C, F;
    long long total;
    double iou;
    const int *clips, *off1;
    const int *g_count, *g_label, *g_track, *g_prev;
    const int *p_count, *p_label, *p_track;
    int *match, *match_gt;
    double *iou_out;
    int *sw, *frag, *frame_tp, *frame_fp, *frame_fn, *seen, *covered, *last_partner;
    int *tp, *fp, *fn, *ids, *frags, *gt_total;
    long long *iou_units;
};

// the track of an instance row as the identity walk takes it: inside the clip's solid rows (base + t < solid), else -1
__device__ __forceinline__ int sco_track(int t, long long base, long long solid) { return t >= 0 && base + t < solid ? t : -1; }

// One workgroup of 1024 threads per clip, the clip's frames in sequence; thread i owns POINT i of the current frame, gt INSTANCE i
// and predicted INSTANCE i.  A frame in four steps with a barrier behind each (and one inside the last, which counts the matches):
//   (1) the point's two labels, clamped, packed into one key ((g+1) << 11 | (p+1)) in LDS; the tables in LDS cleared; the fills of
//       the frame's rows.
//   (2) sizes by LDS integer atomics (|G|, |P|); the overlap c of the point's own pair by a scan over the frame's keys -- every lane
//       reads the same four keys (ds_read_b128, a broadcast) and counts the ones equal to its own.
//   (3) a point whose pair passes c / (|G| + |P| - c) > iou publishes the pair: atomicMax of p into the gt instance's slot, of g into
//       the predicted instance's, of c beside it.  Every point of the pair publishes the same numbers, and by the argument of the
//       header no second pair can pass for either instance, so the slots hold the one partner or -1 whatever the schedule.
//   (4) the instances' threads write their rows; the gt instances' threads walk the identity: the per-track tables live in global
//       memory in the clip's row space, a track is touched by ONE thread per frame (the lowest instance that carries it -- found by a
//       scan over the frame's gt tracks in LDS), and a frame reads what the frames before wrote behind the frame's last barrier.
// The clip's sums stay in registers -- the uniform ones (tp, fp, fn, gt_total) in every thread, ids, frags and the IoU units per
// thread -- and are added up once at the clip's end by LDS integer atomics.  Every barrier is passed by every thread: the clip's
// bounds, a frame's rows and its K are uniform.
__global__ __launch_bounds__(SCO_THREADS) void score_tracks_kernel(const ScoreArgs a)
{
    __shared__ __attribute__((aligned(16))) int s_key[SCO_THREADS];        // the packed labels of point i; 0 behind the frame's points
    __shared__ int s_ng[SCO_THREADS], s_np[SCO_THREADS];                   // |G| of gt instance g, |P| of predicted instance p
    __shared__ int s_mg[SCO_THREADS], s_mp[SCO_THREADS], s_mc[SCO_THREADS];// the partner of gt instance g, of predicted instance p, and the pair's c
    __shared__ int s_trk[SCO_THREADS];                                     // the track of gt instance g, -1 without
    __shared__ int s_sum[2];
    __shared__ unsigned long long s_units;
    const int tid = threadIdx.x;
    const int clip = blockIdx.x;
    int first, end;
    long long base;
    bool clip_ok;
    ft_clip(a.clips, a.off1, clip, a.F, a.total, first, end, base, clip_ok);

    long long top = base, solid = base;                                    // solid: the end of the owned rows that follow base without a gap
    int tp = 0, fp = 0, fn = 0, gt_total = 0;                              // uniform
    int my_ids = 0, my_frags = 0;
    long long my_units = 0;

    for (int f = first; f < end; ++f) {
        const long long start = a.off1[f], stop = a.off1[f + 1];
        int n;
        const bool owns = ft_clip_frame(clip_ok, start, stop, a.total, top, n);
        if (owns && start == solid) solid = stop;
        const bool small = n <= CMF_INST_MAX_POINTS;                       // a larger frame was never clustered: no instances on either side
        const int Kg = small ? ft_clip_frame_instances(owns, a.g_count + f, n) : 0;
        const int Kp = small ? ft_clip_frame_instances(owns, a.p_count + f, n) : 0;
        const size_t row0 = owns ? (size_t)start : 0;

        // ---- (1) labels, cleared tables, fills
        int g = -1, p = -1;
        if (small && tid < n) {
            g = a.g_label[row0 + tid];
            p = a.p_label[row0 + tid];
            g = g >= 0 && g < Kg ? g : -1;
            p = p >= 0 && p < Kp ? p : -1;
        }
        const int key = ((g + 1) << SCO_SHIFT) | (p + 1);
        s_key[tid] = key;
        s_ng[tid] = 0;
        s_np[tid] = 0;
        s_mg[tid] = -1;
        s_mp[tid] = -1;
        s_mc[tid] = 0;
        for (int r = tid; r < n; r += SCO_THREADS) {
            const size_t row = row0 + r;
            a.seen[row] = 0;
            a.covered[row] = 0;
            a.last_partner[row] = -1;
            if (r >= Kp) {
                a.match[row] = -1;
                a.iou_out[row] = 0.0;
            }
            if (r >= Kg) {
                a.match_gt[row] = -1;
                a.sw[row] = 0;
                a.frag[row] = 0;
            }
        }
        __syncthreads();

        // ---- (2) sizes and the overlap of the point's own pair
        const bool both = g >= 0 && p >= 0;
        if (g >= 0) atomicAdd(&s_ng[g], 1);
        if (p >= 0) atomicAdd(&s_np[p], 1);
        int c = 0;
        if (both) {
            const int4 *keys = reinterpret_cast<const int4 *>(s_key);
            const int quads = (n + 3) >> 2;                                // n <= 1024 here; the keys behind n are 0, no pair's key
            for (int q = 0; q < quads; ++q) {
                const int4 k = keys[q];
                c += (k.x == key) + (k.y == key) + (k.z == key) + (k.w == key);
            }
        }
        __syncthreads();

        // ---- (3) the pairs that pass
        if (both) {
            const int u = s_ng[g] + s_np[p] - c;                           // >= c >= 1: the point itself
            if ((double)c / (double)u > a.iou) {
                atomicMax(&s_mg[g], p);
                atomicMax(&s_mp[p], g);
                atomicMax(&s_mc[p], c);
            }
        }
        __syncthreads();

        // ---- (4) the instances' rows
        if (tid < Kp) {
            const int mg = s_mp[tid];
            double q = 0.0;
            if (mg >= 0) {
                const int cc = s_mc[tid];
                q = (double)cc / (double)(s_ng[mg] + s_np[tid] - cc);      // the same division from the same operands
                my_units += (long long)floor(q * 1073741824.0);
            }
            a.match[row0 + tid] = mg >= 0 ? (int)(row0 + mg) : -1;
            a.iou_out[row0 + tid] = q;
        }
        const int mine = tid < Kg ? s_mg[tid] : -1;                        // the predicted instance this gt instance matched
        int t = -1;
        if (tid < Kg) {
            a.match_gt[row0 + tid] = mine >= 0 ? (int)(row0 + mine) : -1;
            t = sco_track(a.g_track[row0 + tid], base, solid);
        }
        s_trk[tid] = t;
        const int frame_tp = __syncthreads_count(mine >= 0);               // also: s_trk and the fills of the per-track rows are visible
        if (t >= 0) {
            bool ident = true;
            for (int j = 0; j < tid; ++j) ident = ident && s_trk[j] != t;   // a track counts once per frame, for its lowest instance
            int sw = 0, fr = 0;
            if (ident) {
                const size_t tr = (size_t)base + t;                         // < solid: a row of an owned frame up to this one
                a.seen[tr] += 1;
                if (mine >= 0) {
                    const int u = sco_track(a.p_track[row0 + mine], base, solid);
                    const int cv = a.covered[tr];
                    if (cv > 0) {                                          // the track was matched before
                        sw = a.last_partner[tr] != u;
                        const long long before = a.g_prev[row0 + tid];
                        const bool linked = before >= base && before < (long long)row0 && before < solid;
                        fr = !(linked && a.match_gt[linked ? before : 0] >= 0);
                    }
                    a.covered[tr] = cv + 1;
                    a.last_partner[tr] = u;
                }
            }
            a.sw[row0 + tid] = sw;
            a.frag[row0 + tid] = fr;
            my_ids += sw;
            my_frags += fr;
        } else if (tid < Kg) {
            a.sw[row0 + tid] = 0;
            a.frag[row0 + tid] = 0;
        }
        if (tid == 0) {
            a.frame_tp[f] = frame_tp;
            a.frame_fp[f] = Kp - frame_tp;
            a.frame_fn[f] = Kg - frame_tp;
        }
        tp += frame_tp;
        fp += Kp - frame_tp;
        fn += Kg - frame_tp;
        gt_total += Kg;
        __syncthreads();                                                   // the next frame overwrites the tables and reads this one's rows
    }

    // ---- the clip's sums
    if (tid == 0) {
        s_sum[0] = 0;
        s_sum[1] = 0;
        s_units = 0ull;
    }
    __syncthreads();
    if (my_ids) atomicAdd(&s_sum[0], my_ids);
    if (my_frags) atomicAdd(&s_sum[1], my_frags);
    if (my_units) atomicAdd(&s_units, (unsigned long long)my_units);
    __syncthreads();
    if (tid == 0) {
        a.tp[clip] = tp;
        a.fp[clip] = fp;
        a.fn[clip] = fn;
        a.ids[clip] = s_sum[0];
        a.frags[clip] = s_sum[1];
        a.gt_total[clip] = gt_total;
        a.iou_units[clip] = (long long)s_units;
    }
}

}  // namespace

extern "C" int cmf_score_tracks(int nclips, int nframes, const int *clips, const int *off1, long long total, double iou_min,
                                const int *gt_count, const int *gt_label, const int *gt_track, const int *gt_prev_row,
                                const int *pred_count, const int *pred_label, const int *pred_track, int *match, int *match_gt,
                                double *iou, int *switches, int *frag, int *frame_tp, int *frame_fp, int *frame_fn, int *seen,
                                int *covered, int *last_partner, int *tp, int *fp, int *fn, int *ids, int *frags, int *gt_total,
                                long long *iou_units, void *stream)
{
    CMF_CHECK_ARG(nclips >= 0 && nframes >= 1 && total >= 0 && total <= 2147483647LL);
    CMF_CHECK_ARG(iou_min >= 0.5 && iou_min < 1.0);                              // a NaN fails both
    if (nclips == 0) return 0;
    CMF_CHECK_ARG(clips && off1 && gt_count && pred_count && frame_tp && frame_fp && frame_fn);
    CMF_CHECK_ARG(tp && fp && fn && ids && frags && gt_total && iou_units);
    CMF_CHECK_ARG(total == 0 || (gt_label && gt_track && gt_prev_row && pred_label && pred_track && match && match_gt && iou && switches &&
                                 frag && seen && covered && last_partner));
    ScoreArgs a{nclips, nframes, total, iou_min, clips, off1, gt_count, gt_label, gt_track, gt_prev_row, pred_count, pred_label, pred_track,
                match, match_gt, iou, switches, frag, frame_tp, frame_fp, frame_fn, seen, covered, last_partner,
                tp, fp, fn, ids, frags, gt_total, iou_units};
    hipLaunchKernelGGL(score_tracks_kernel, dim3(nclips), dim3(SCO_THREADS), 0, (hipStream_t)stream, a);
    return cmf_launch_status();
}
