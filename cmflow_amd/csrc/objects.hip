// Per-track object states of a test run (cmflow_amd/objects.py): over the matches of every track that
// cmf_track_instances formed, a constant-velocity Kalman filter forwards and a Rauch-Tung-Striebel smoother backwards in the clip's
// axes, then per match the smoothed position and velocity back in the frame's own axes, a heading from the velocity and a box
// oriented along it.  A DEFINITION, stated in include/cmflow_hip.h and restated in numpy, bit for bit, by tests/objects_ref.py:
// float64 from the float32 inputs, + - * / and sqrt only, a fixed operation order, no contraction anywhere in this file, and no
// dependence on the order in which threads run.
#include "frame_tables.h"

#pragma clang fp contract(off)

namespace {

constexpr int OBJ_THREADS = 256;

struct StateArgs {
    int C, F, ld;
    long long total;
    double rp, rd, q, min_disp2;
    const int *clips, *off1, *count, *label, *track, *prev_row, *gap;
    const float *centroid, *disp, *tab1;
    const double *poses;
    int *row_frame, *next_row, *heading_src;
    double *filt, *fcov, *state, *scov;
    float *pos, *vel, *heading, *box_center, *box_size;
};

// A clip is taken in chunks of OBJ_CHUNK frames; a chunk's table also holds the OBJ_REACH frames behind it, where the successors of
// its last frames are searched.  OBJ_GROUPS frames are worked on at a time, OBJ_LANES threads each.
constexpr int OBJ_CHUNK = 256, OBJ_REACH = CMF_TRACK_MAX_GAP + 1, OBJ_TABLE = OBJ_CHUNK + OBJ_REACH;
constexpr int OBJ_LANES = 16, OBJ_GROUPS = OBJ_THREADS / OBJ_LANES;

struct FrameTable {
    int off[OBJ_TABLE + 1], cnt[OBJ_TABLE];                                // the raw offsets and counts of the frames f0 ..
    int start[OBJ_TABLE], n[OBJ_TABLE], K[OBJ_TABLE];                      // a frame that owns no rows: 0, 0, 0
    long long top;                                                         // top behind the chunk's last frame
};

// The rows of the frames f0 .. f0 + OBJ_TABLE - 1 of a clip (cut at its end), walked by ft_clip_frame of frame_tables.h as the tracker
// walks them.  The loads are spread over the workgroup, the walk itself (top is sequential) is thread
// 0's over LDS.  -> top behind the chunk proper.  Called by every thread; three barriers.
__device__ __forceinline__ long long obj_chunk(const StateArgs &a, bool clip_ok, int f0, int end, long long top, FrameTable &t)
{
    const int tid = threadIdx.x;
    const int m = end - f0 < OBJ_TABLE ? end - f0 : OBJ_TABLE;
    __syncthreads();                                                       // whoever still reads the table of the chunk before
    for (int i = tid; i <= m; i += OBJ_THREADS) t.off[i] = a.off1[f0 + i];
    for (int i = tid; i < m; i += OBJ_THREADS) t.cnt[i] = a.count[f0 + i];
    __syncthreads();
    if (tid == 0) {
        long long at = top, behind = top;
        for (int i = 0; i < m; ++i) {
            const long long start = t.off[i], stop = t.off[i + 1];
            int n;
            const bool owns = ft_clip_frame(clip_ok, start, stop, a.total, at, n);
            t.start[i] = owns ? (int)start : 0;
            t.n[i] = n;
            t.K[i] = ft_clip_frame_instances(owns, t.cnt + i, n);
            if (i < OBJ_CHUNK) behind = at;
        }
        t.top = behind;
    }
    __syncthreads();
    return t.top;
}

// W_f, the pose of scan 1 of frame f (upper three rows): poses[f-1], the identity as numbers at the clip's first frame
__device__ __forceinline__ void obj_scan1_pose(const StateArgs &a, int f, int first, double W[12])
{
    if (f == first) {
        for (int e = 0; e < 12; ++e) W[e] = (e == 0 || e == 5 || e == 10) ? 1.0 : 0.0;
    } else {
        const double *src = a.poses + (size_t)(f - 1) * 16;
        for (int e = 0; e < 12; ++e) W[e] = src[e];
    }
}

__device__ __forceinline__ double obj_gap(int gap)
{
    return (double)(gap < 1 ? 1 : gap > CMF_TRACK_MAX_GAP + 1 ? CMF_TRACK_MAX_GAP + 1 : gap);
}

// PREDICT of the header: the same expressions for the filter and, formed again from the filtered values, for the smoother
__device__ __forceinline__ void obj_predict(double g, double q, const double p[3], const double v[3], double ca, double cb, double cc,
                                            double pm[3], double &am, double &bm, double &cm)
{
    for (int r = 0; r < 3; ++r) pm[r] = p[r] + g * v[r];
    am = (ca + g * ((2.0 * cb) + g * cc)) + (q * ((g * g) * g)) / 3.0;
    bm = (cb + g * cc) + (q * (g * g)) / 2.0;
    cm = cc + q * g;
}

// One workgroup per clip, three phases with a barrier between them; each phase takes the clip in chunks of frames whose rows are
// tabled in LDS (obj_chunk), OBJ_GROUPS frames at a time with OBJ_LANES threads each -- a frame holds a handful of instances, so
// frames side by side keep the workgroup busy where one frame after the other leaves it idle.  (1) links: the thread of an instance
// row finds the row's successor by a search over the instance rows of the next CMF_TRACK_MAX_GAP + 1 frames, and the rows behind K
// get their fills.  (2) chains: the thread of a row that is a head walks its chain forwards (filter) and backwards (smoother) --
// sequential per track, parallel over the tracks, no barrier inside, so a wave whose heads are done goes on.  (3) boxes: the thread
// of an instance row reads its smoothed state, turns it into the frame's axes and scans the frame's labels for its members.  Every
// barrier is passed by every thread: the clip's bounds and the chunk loops are uniform.
__global__ __launch_bounds__(OBJ_THREADS) void track_states_kernel(const StateArgs a)
{
    __shared__ FrameTable tab;
    const int tid = threadIdx.x, group = tid / OBJ_LANES, lane = tid % OBJ_LANES;
    const int clip = blockIdx.x;
    int first, end;
    long long base;
    bool clip_ok;
    ft_clip(a.clips, a.off1, clip, a.F, a.total, first, end, base, clip_ok);
    const int N = end - first;

    // ---- (1) links and fills
    long long top = base;
    for (int f0 = first; f0 < end; f0 += OBJ_CHUNK) {
      top = obj_chunk(a, clip_ok, f0, end, top, tab);
      const int frames = end - f0 < OBJ_CHUNK ? end - f0 : OBJ_CHUNK;
      for (int fi = group; fi < frames; fi += OBJ_GROUPS) {
        const int f = f0 + fi, start = tab.start[fi], n = tab.n[fi], K = tab.K[fi];
        const int reach = end - 1 - f > OBJ_REACH ? OBJ_REACH : end - 1 - f;   // fi + reach < the table's frames
        for (int j = lane; j < n; j += OBJ_LANES) {
            const size_t row = (size_t)start + j;
            if (j < K) {
                const int mine = a.track[row];
                int next = -1;
                for (int d = 1; d <= reach && next < 0; ++d) {
                    const int start2 = tab.start[fi + d], K2 = tab.K[fi + d];
                    for (int j2 = 0; j2 < K2; ++j2) {                      // no early exit: the loads of a frame do not wait for one another
                        const size_t row2 = (size_t)start2 + j2;
                        if (next < 0 && a.prev_row[row2] == (int)row && a.track[row2] == mine) next = (int)row2;
                    }
                }
                a.row_frame[row] = f;
                a.next_row[row] = next;
            } else {
                a.row_frame[row] = -1;
                a.next_row[row] = -1;
                a.heading_src[row] = -1;
                for (int e = 0; e < 6; ++e) {
                    a.filt[6 * row + e] = 0.0;
                    a.state[6 * row + e] = 0.0;
                }
                for (int e = 0; e < 3; ++e) {
                    a.fcov[3 * row + e] = 0.0;
                    a.scov[3 * row + e] = 0.0;
                    a.pos[3 * row + e] = 0.0f;
                    a.vel[3 * row + e] = 0.0f;
                    a.box_center[3 * row + e] = 0.0f;
                    a.box_size[3 * row + e] = 0.0f;
                }
                a.heading[2 * row] = 0.0f;
                a.heading[2 * row + 1] = 0.0f;
            }
        }
      }
    }
    __syncthreads();

    // ---- (2) chains: the filter forwards, the smoother backwards
    top = base;
    for (int f0 = first; f0 < end; f0 += OBJ_CHUNK) {
      top = obj_chunk(a, clip_ok, f0, end, top, tab);
      const int frames = end - f0 < OBJ_CHUNK ? end - f0 : OBJ_CHUNK;
      for (int fi = group; fi < frames; fi += OBJ_GROUPS) {
        const int f = f0 + fi, start = tab.start[fi], K = tab.K[fi];
        for (int j = lane; j < K; j += OBJ_LANES) {
            const long long head = (long long)start + j;
            const long long before = a.prev_row[head];
            if (before >= base && before < start && a.next_row[before] == (int)head) continue;         // not a head: its chain's head walks it
            double p[3], v[3], ca = 0.0, cb = 0.0, cc = 0.0;
            long long k = head;
            int steps = 0;
            for (;;) {
                int fk = steps == 0 ? f : a.row_frame[k];
                fk = fk < first ? first : fk > end - 1 ? end - 1 : fk;    // only clips that overlap (the caller's error) leave another clip's frame here
                double W[12];
                obj_scan1_pose(a, fk, first, W);
                const double *A = a.poses + (size_t)fk * 16;
                const double c0 = (double)a.centroid[3 * k], c1 = (double)a.centroid[3 * k + 1], c2 = (double)a.centroid[3 * k + 2];
                const double d0 = (double)a.disp[3 * k], d1 = (double)a.disp[3 * k + 1], d2 = (double)a.disp[3 * k + 2];
                double zp[3], zd[3];
                for (int r = 0; r < 3; ++r) {
                    zp[r] = ((W[4 * r] * c0 + W[4 * r + 1] * c1) + W[4 * r + 2] * c2) + W[4 * r + 3];
                    zd[r] = (A[4 * r] * d0 + A[4 * r + 1] * d1) + A[4 * r + 2] * d2;
                }
                if (steps == 0) {
                    for (int r = 0; r < 3; ++r) {
                        p[r] = zp[r];
                        v[r] = zd[r];
                    }
                    ca = a.rp; cb = 0.0; cc = a.rd;
                } else {
                    const double g = obj_gap(a.gap[k]);
                    double pm[3], am, bm, cm;
                    obj_predict(g, a.q, p, v, ca, cb, cc, pm, am, bm, cm);
                    const double s11 = am + a.rp, s12 = bm, s22 = cm + a.rd;
                    const double det = s11 * s22 - s12 * s12;
                    const double k11 = (am * s22 - bm * s12) / det, k12 = (bm * s11 - am * s12) / det;
                    const double k21 = (bm * s22 - cm * s12) / det, k22 = (cm * s11 - bm * s12) / det;
                    for (int r = 0; r < 3; ++r) {
                        const double ep = zp[r] - pm[r], ev = zd[r] - v[r];
                        p[r] = pm[r] + (k11 * ep + k12 * ev);
                        v[r] = v[r] + (k21 * ep + k22 * ev);
                    }
                    ca = am - (k11 * am + k12 * bm);
                    cb = bm - (k11 * bm + k12 * cm);
                    cc = cm - (k21 * bm + k22 * cm);
                }
                for (int r = 0; r < 3; ++r) {
                    a.filt[6 * k + r] = p[r];
                    a.filt[6 * k + 3 + r] = v[r];
                }
                a.fcov[3 * k] = ca; a.fcov[3 * k + 1] = cb; a.fcov[3 * k + 2] = cc;
                steps += 1;
                const long long nk = a.next_row[k];
                if (nk <= k || nk >= a.total || steps >= N) break;         // -1: the chain's end; a link only ever ascends, inside the tables
                k = nk;
            }
            // k: the chain's last row; (p, v, ca, cb, cc) from here on: the SMOOTHED values of the row behind
            for (int r = 0; r < 3; ++r) {
                a.state[6 * k + r] = p[r];
                a.state[6 * k + 3 + r] = v[r];
            }
            a.scov[3 * k] = ca; a.scov[3 * k + 1] = cb; a.scov[3 * k + 2] = cc;
            for (int back = steps - 1; back > 0; --back) {
                const long long jrow = a.prev_row[k];                      // the row step 1 linked k to: prev_row[next_row[j]] == j
                if (jrow < base || jrow >= k) break;
                const double g = obj_gap(a.gap[k]);
                double fp[3], fv[3];
                for (int r = 0; r < 3; ++r) {
                    fp[r] = a.filt[6 * jrow + r];
                    fv[r] = a.filt[6 * jrow + 3 + r];
                }
                const double fa = a.fcov[3 * jrow], fb = a.fcov[3 * jrow + 1], fc = a.fcov[3 * jrow + 2];
                double pm[3], am, bm, cm;
                obj_predict(g, a.q, fp, fv, fa, fb, fc, pm, am, bm, cm);
                const double m11 = fa + g * fb, m12 = fb, m21 = fb + g * fc, m22 = fc;
                const double dm = am * cm - bm * bm;
                const double c11 = (m11 * cm - m12 * bm) / dm, c12 = (m12 * am - m11 * bm) / dm;
                const double c21 = (m21 * cm - m22 * bm) / dm, c22 = (m22 * am - m21 * bm) / dm;
                for (int r = 0; r < 3; ++r) {
                    const double dp = p[r] - pm[r], dv = v[r] - fv[r];
                    p[r] = fp[r] + (c11 * dp + c12 * dv);
                    v[r] = fv[r] + (c21 * dp + c22 * dv);
                }
                const double da = ca - am, db = cb - bm, dc = cc - cm;
                const double e11 = c11 * da + c12 * db, e12 = c11 * db + c12 * dc, e21 = c21 * da + c22 * db, e22 = c21 * db + c22 * dc;
                ca = fa + (e11 * c11 + e12 * c12);
                cb = fb + (e11 * c21 + e12 * c22);
                cc = fc + (e21 * c21 + e22 * c22);
                k = jrow;
                for (int r = 0; r < 3; ++r) {
                    a.state[6 * k + r] = p[r];
                    a.state[6 * k + 3 + r] = v[r];
                }
                a.scov[3 * k] = ca; a.scov[3 * k + 1] = cb; a.scov[3 * k + 2] = cc;
            }
        }
      }
    }
    __syncthreads();

    // ---- (3) into the frame's axes, the heading, the box
    top = base;
    for (int f0 = first; f0 < end; f0 += OBJ_CHUNK) {
      top = obj_chunk(a, clip_ok, f0, end, top, tab);
      const int frames = end - f0 < OBJ_CHUNK ? end - f0 : OBJ_CHUNK;
      for (int fi = group; fi < frames; fi += OBJ_GROUPS) {
        const int f = f0 + fi, start = tab.start[fi], n = tab.n[fi], K = tab.K[fi];
        if (lane >= K) continue;
        double W[12];
        obj_scan1_pose(a, f, first, W);
        for (int j = lane; j < K; j += OBJ_LANES) {
            const size_t row = (size_t)start + j;
            double x[3], v[3], P[3], V[3];
            for (int r = 0; r < 3; ++r) {
                x[r] = a.state[6 * row + r];
                v[r] = a.state[6 * row + 3 + r];
            }
            for (int r = 0; r < 3; ++r) {
                const double ti = -((W[r] * W[3] + W[4 + r] * W[7]) + W[8 + r] * W[11]);
                P[r] = ((W[r] * x[0] + W[4 + r] * x[1]) + W[8 + r] * x[2]) + ti;
                V[r] = (W[r] * v[0] + W[4 + r] * v[1]) + W[8 + r] * v[2];
                a.pos[3 * row + r] = (float)P[r];
                a.vel[3 * row + r] = (float)V[r];
            }
            const double s2 = V[0] * V[0] + V[1] * V[1];
            float h0 = 1.0f, h1 = 0.0f;
            int src = 0;
            if (s2 >= a.min_disp2 && s2 > 0.0) {
                const double s = sqrt(s2);
                h0 = (float)(V[0] / s);
                h1 = (float)(V[1] / s);
                src = 1;
            }
            a.heading[2 * row] = h0;
            a.heading[2 * row + 1] = h1;
            a.heading_src[row] = src;
            const double hx = (double)h0, hy = (double)h1;
            const float cf0 = a.centroid[3 * row], cf1 = a.centroid[3 * row + 1], cf2 = a.centroid[3 * row + 2];
            const double c0 = (double)cf0, c1 = (double)cf1;
            bool any = false;
            double amin = 0.0, amax = 0.0, bmin = 0.0, bmax = 0.0;
            float lo = 0.0f, hi = 0.0f;
            for (int i = 0; i < n; ++i) {
                if (a.label[(size_t)start + i] != j) continue;
                const float *pt = a.tab1 + ((size_t)start + i) * a.ld;
                const double dx = (double)pt[0] - c0, dy = (double)pt[1] - c1;
                const double ai = hx * dx + hy * dy, bi = (-hy) * dx + hx * dy;
                const float z = pt[2];
                if (!any) {
                    any = true;
                    amin = ai; amax = ai; bmin = bi; bmax = bi; lo = z; hi = z;
                } else {
                    if (ai < amin) amin = ai;
                    if (ai > amax) amax = ai;
                    if (bi < bmin) bmin = bi;
                    if (bi > bmax) bmax = bi;
                    if (z < lo) lo = z;
                    if (z > hi) hi = z;
                }
            }
            if (any) {
                const double ma = (amin + amax) / 2.0, mb = (bmin + bmax) / 2.0;
                a.box_size[3 * row] = (float)(amax - amin);
                a.box_size[3 * row + 1] = (float)(bmax - bmin);
                a.box_size[3 * row + 2] = (float)((double)hi - (double)lo);
                a.box_center[3 * row] = (float)(c0 + (ma * hx - mb * hy));
                a.box_center[3 * row + 1] = (float)(c1 + (ma * hy + mb * hx));
                a.box_center[3 * row + 2] = (float)(((double)lo + (double)hi) / 2.0);
            } else {
                a.box_size[3 * row] = 0.0f; a.box_size[3 * row + 1] = 0.0f; a.box_size[3 * row + 2] = 0.0f;
                a.box_center[3 * row] = cf0; a.box_center[3 * row + 1] = cf1; a.box_center[3 * row + 2] = cf2;
            }
        }
      }
    }
}

}  // namespace

extern "C" int cmf_track_states(int nclips, int nframes, const int *clips, const int *off1, long long total, const int *count,
                                const int *label, const float *centroid, const float *disp, const int *track, const int *prev_row,
                                const int *gap, const float *tab1, int ld_tab, const double *poses, double rp, double rd, double q,
                                double min_disp2, int *row_frame, int *next_row, double *filt, double *fcov, double *state,
                                double *scov, float *pos, float *vel, float *heading, int *heading_src, float *box_center,
                                float *box_size, void *stream)
{
    CMF_CHECK_ARG(nclips >= 0 && nframes >= 1 && total >= 0 && total <= 2147483647LL && ld_tab >= 3);
    CMF_CHECK_ARG(rp > 0.0 && rd > 0.0 && q >= 0.0 && min_disp2 >= 0.0);    // a NaN fails every one of these
    if (nclips == 0) return 0;
    CMF_CHECK_ARG(clips && off1 && count && poses);
    CMF_CHECK_ARG(total == 0 || (label && centroid && disp && track && prev_row && gap && tab1 && row_frame && next_row && filt && fcov &&
                                 state && scov && pos && vel && heading && heading_src && box_center && box_size));
    StateArgs a{nclips, nframes, ld_tab, total, rp, rd, q, min_disp2, clips, off1, count, label, track, prev_row, gap, centroid, disp, tab1,
                poses, row_frame, next_row, heading_src, filt, fcov, state, scov, pos, vel, heading, box_center, box_size};
    hipLaunchKernelGGL(track_states_kernel, dim3(nclips), dim3(OBJ_THREADS), 0, (hipStream_t)stream, a);
    return cmf_launch_status();
}
