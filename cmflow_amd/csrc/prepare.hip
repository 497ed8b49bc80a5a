// cmf_prepare_*: from raw radar scans to the packed tables of a DeviceSplit (cmflow_amd/prepare.py) -- the arithmetic of the
// reference's offline preprocess step (preprocess/utils/get_flow_samples.py: FOV + height filter, foreground from box tracks, rigid
// flow, the gt / pseudo label rules) on whole batches of scans and frame pairs.  DESIGN.md section 15.
//
//   cmf_prepare_count   one workgroup per scan: the input filter on every raw row, an ORDERED prefix over workgroup-sized chunks
//                       (ballot per wave, four wave totals in LDS) -> per raw row its position among the kept rows of its scan
//                       (-1: dropped) and its pixel (u, v); per scan the kept count.
//   cmf_prepare_pairs   one workgroup per pair: the kept rows of both scans go to the pair's tab1 / tab2 rows (xyz, features, u, v,
//                       optical flow); then the boxes in record order -- a reduction over the box's points (any inside? any in-box
//                       flow of 3 m or more?) and a conditional write; then the label rule of the mode.  Thread t owns the points
//                       t, t + 256, ... of cloud 1 from the boxes on, so a point's foreground label (kept as float32 in its
//                       table row, as the reference keeps it) is read and written by one thread only.
//   cmf_prepare_scans   the inference front end: the same filter, kept rows written straight into forward_ragged's padded layout.
//
// Every decision (pixel, in-box, 3 m gate, 0.05 m moving rule) is taken in float64 on the float32 coordinates, as numpy takes it in
// the reference, and this file is built with -ffp-contract=off: a fused multiply-add would round differently from the host's
// separately rounded products and could move a compare.  Values are rounded to float32 once, at the store.
#include "cmf_common.h"
#include "../../include/cmflow_hip.h"

namespace {

constexpr int PREP_THREADS = 256, PREP_WAVES = PREP_THREADS / CMF_WAVE;
constexpr int PREP_COLS1 = 14, PREP_COLS2 = 6;
constexpr int PREP_SLOTS = CMF_DRAW_MAX_POINTS / PREP_THREADS;            // points of cloud 1 a thread owns: 64, one bit each
static_assert(PREP_SLOTS <= 64, "the foreground bits of a thread's points live in one 64-bit register");

struct FilterArgs {
    int C, per_scan, W, H;
    double zlo, zhi;
    const float *scans;
    const int *scan_off;
    const double *tcr, *proj;                                              // (S or 1, 16), (S or 1, 12)
};

// The input filter on one raw row (get_flow_samples.py:63-70, optical_flow.py:77-89, transformations.py:285-328):
// p_cam = T [x y z 1], uvw = P p_cam, (u, v) = rint(uvw / w) half to even, kept when 0 < u <= W, 0 < v <= H, zlo <= z <= zhi.  No
// depth test (the reference has none).  w zero or not finite: dropped (undefined in the reference); NaN fails every compare.
__device__ inline bool prep_keep(const float *row, const double *T, const double *P, const FilterArgs &a, int &u, int &v)
{
    const double x = row[0], y = row[1], z = row[2];
    double c[4], q[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = ((T[4 * i] * x + T[4 * i + 1] * y) + T[4 * i + 2] * z) + T[4 * i + 3];
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = ((P[4 * i] * c[0] + P[4 * i + 1] * c[1]) + P[4 * i + 2] * c[2]) + P[4 * i + 3] * c[3];
    if (!isfinite(q[2]) || q[2] == 0.0) return false;
    const double ru = rint(q[0] / q[2]), rv = rint(q[1] / q[2]);
    if (!(ru > 0.0 && ru <= (double)a.W && rv > 0.0 && rv <= (double)a.H)) return false;
    if (!(z >= a.zlo && z <= a.zhi)) return false;
    u = (int)ru;
    v = (int)rv;
    return true;
}

// The filter over scan s in chunks of PREP_THREADS rows with an ordered prefix: emit(raw row, rank or -1, u, v) for every row of the
// scan, rank = the row's position among the scan's kept rows (scan order).  All threads of the workgroup call it; -> kept count.
template <typename Emit>
__device__ inline int prep_filter_scan(const FilterArgs &a, int s, Emit emit)
{
    __shared__ int wave_tot[PREP_WAVES];
    const int t = threadIdx.x, lane = t & (CMF_WAVE - 1), wv = t / CMF_WAVE;
    const long long r0 = a.scan_off[s], r1 = a.scan_off[s + 1];
    const double *T = a.tcr + (a.per_scan ? (size_t)s * 16 : 0), *P = a.proj + (a.per_scan ? (size_t)s * 12 : 0);
    int base = 0;
    for (long long c0 = r0; c0 < r1; c0 += PREP_THREADS) {
        const long long r = c0 + t;
        int u = 0, v = 0;
        const bool k = r < r1 && prep_keep(a.scans + (size_t)r * a.C, T, P, a, u, v);
        const unsigned long long m = __ballot(k);
        if (lane == 0) wave_tot[wv] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < PREP_WAVES; ++w) {
            const int c = wave_tot[w];
            total += c;
            before += w < wv ? c : 0;
        }
        if (r < r1) emit(r, k ? base + before + __popcll(m & ((1ull << lane) - 1ull)) : -1, u, v);
        base += total;
        __syncthreads();                                                   // wave_tot is written again in the next chunk
    }
    return base;
}

struct CountArgs { FilterArgs f; int *keep, *uv, *count; };

__global__ __launch_bounds__(PREP_THREADS) void prepare_count_kernel(const CountArgs a)
{
    const int s = blockIdx.x;
    const int n = prep_filter_scan(a.f, s, [&](long long r, int rank, int u, int v) {
        a.keep[r] = rank;
        a.uv[2 * r] = u;
        a.uv[2 * r + 1] = v;
    });
    if (threadIdx.x == 0) a.count[s] = n;
}

struct ScansArgs { FilterArgs f; int nmax; float *pc, *ft; int *n; };

__global__ __launch_bounds__(PREP_THREADS) void prepare_scans_kernel(const ScansArgs a)
{
    const int s = blockIdx.x, N = a.nmax;
    float *pc = a.pc + (size_t)s * 3 * N, *ft = a.ft + (size_t)s * 3 * N;
    const int cnt = prep_filter_scan(a.f, s, [&](long long r, int rank, int, int) {
        if (rank < 0 || rank >= N) return;                                 // a too-small nmax truncates the scan (n says so)
        const float *row = a.f.scans + (size_t)r * a.f.C;
        pc[rank] = row[0];
        pc[N + rank] = row[1];
        pc[2 * N + rank] = row[2];
        ft[rank] = row[4];                                                 // v_r RCS RCS (dataset/vod.py:62-63)
        ft[N + rank] = row[3];
        ft[2 * N + rank] = row[3];
    });
    const int n = min(cnt, N);
    for (int e = threadIdx.x; e < 3 * (N - n); e += PREP_THREADS) {        // padded slots: exact zeros
        const int c = e / (N - n), j = n + (e - c * (N - n));
        pc[c * N + j] = 0.0f;
        ft[c * N + j] = 0.0f;
    }
    if (threadIdx.x == 0) a.n[s] = n;
}

struct PairsArgs {
    int F, C, mode, W, H;
    const float *scans;
    const int *scan_off, *keep, *uv, *pairs, *off1, *off2;
    const double *tinv, *boxes;
    const int *box_off;
    const float *const *flow;
    float *tab1, *tab2;
};

// offsets into a box record of CMF_PREP_BOX_DOUBLES doubles
constexpr int BOX_C = 0, BOX_R = 3, BOX_HALF = 12, BOX_T = 15, BOX_SCORE = 31;

// p in the CLOSED oriented box: |(p - c) . axis_a| <= half_a for the three columns of R
__device__ inline bool prep_in_box(const double *B, double x, double y, double z)
{
    const double dx = x - B[BOX_C], dy = y - B[BOX_C + 1], dz = z - B[BOX_C + 2];
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double d = (dx * B[BOX_R + a] + dy * B[BOX_R + 3 + a]) + dz * B[BOX_R + 6 + a];
        in = in && fabs(d) <= B[BOX_HALF + a];
    }
    return in;
}

// (T [p 1])[:3] - p for a row-major 4 x 4 T
__device__ inline void prep_flow(const double *T, double x, double y, double z, double f[3])
{
    f[0] = (((T[0] * x + T[1] * y) + T[2] * z) + T[3]) - x;
    f[1] = (((T[4] * x + T[5] * y) + T[6] * z) + T[7]) - y;
    f[2] = (((T[8] * x + T[9] * y) + T[10] * z) + T[11]) - z;
}

__global__ __launch_bounds__(PREP_THREADS) void prepare_pairs_kernel(const PairsArgs a)
{
    const int f = blockIdx.x, t = threadIdx.x;
    const int s1 = a.pairs[2 * f], s2 = a.pairs[2 * f + 1];
    const long long o1 = a.off1[f], o2 = a.off2[f];
    const int n1 = a.off1[f + 1] - a.off1[f], n2 = a.off2[f + 1] - a.off2[f];
    float *t1 = a.tab1 + (size_t)o1 * PREP_COLS1, *t2 = a.tab2 + (size_t)o2 * PREP_COLS2;
    const bool pseudo = a.mode == CMF_PREP_MODE_PSEUDO;
    const float *img = pseudo && a.flow ? a.flow[f] : nullptr;

    // ---- the kept rows of both scans, in scan order (copies; label and mask columns start as background) ----
    for (long long r = (long long)a.scan_off[s2] + t; r < a.scan_off[s2 + 1]; r += PREP_THREADS) {
        const int k = a.keep[r];
        if (k < 0 || k >= n2) continue;
        const float *row = a.scans + (size_t)r * a.C;
        float *dst = t2 + (size_t)k * PREP_COLS2;
        dst[0] = row[0]; dst[1] = row[1]; dst[2] = row[2];
        dst[3] = row[4]; dst[4] = row[3]; dst[5] = row[3];
    }
    for (long long r = (long long)a.scan_off[s1] + t; r < a.scan_off[s1 + 1]; r += PREP_THREADS) {
        const int k = a.keep[r];
        if (k < 0 || k >= n1) continue;
        const float *row = a.scans + (size_t)r * a.C;
        float *dst = t1 + (size_t)k * PREP_COLS1;
        dst[0] = row[0]; dst[1] = row[1]; dst[2] = row[2];
        dst[3] = row[4]; dst[4] = row[3]; dst[5] = row[3];
        dst[6] = dst[7] = dst[8] = 0.0f;
        dst[9] = 0.0f;                                                     // the box confidence until the label rule turns it into the mask
        const int u = a.uv[2 * r], v = a.uv[2 * r + 1];
        dst[10] = pseudo ? (float)u : 0.0f;
        dst[11] = pseudo ? (float)v : 0.0f;
        float g0 = 0.0f, g1 = 0.0f;
        if (img) {                                                         // opt_flow[v - 1, u - 1] (optical_flow.py:66); the filter put (u, v) inside
            const size_t px = (size_t)min(max(v - 1, 0), a.H - 1) * a.W + min(max(u - 1, 0), a.W - 1);
            g0 = img[2 * px];
            g1 = img[2 * px + 1];
        }
        dst[12] = g0;
        dst[13] = g1;
    }
    __syncthreads();                                                       // rows written by other threads are read below

    // ---- foreground from the boxes, in record order; a later box overwrites an earlier one ----
    const int slots = min((n1 - t + PREP_THREADS - 1) / PREP_THREADS, PREP_SLOTS);     // this thread's points: t + 256 k < n1
    unsigned long long fg = 0;
    for (int b = a.box_off[f]; b < a.box_off[f + 1]; ++b) {
        const double *B = a.boxes + (size_t)b * CMF_PREP_BOX_DOUBLES;
        unsigned long long in = 0;
        int far = 0;
        for (int k = 0; k < slots; ++k) {
            const float *p = t1 + (size_t)(t + k * PREP_THREADS) * PREP_COLS1;
            const double x = p[0], y = p[1], z = p[2];
            if (!prep_in_box(B, x, y, z)) continue;
            in |= 1ull << k;
            double fl[3];
            prep_flow(B + BOX_T, x, y, z, fl);
            far |= !(sqrt((fl[0] * fl[0] + fl[1] * fl[1]) + fl[2] * fl[2]) < 3.0);
        }
        const int any_in = __syncthreads_or(in != 0), any_far = __syncthreads_or(far);
        if (!any_in || any_far) continue;                                  // empty box, or a track jump of 3 m or more: no label
        const float conf = (float)B[BOX_SCORE];
        for (int k = 0; k < slots; ++k) {
            if (!(in >> k & 1)) continue;
            float *p = t1 + (size_t)(t + k * PREP_THREADS) * PREP_COLS1;
            double fl[3];
            prep_flow(B + BOX_T, (double)p[0], (double)p[1], (double)p[2], fl);
            p[6] = (float)fl[0]; p[7] = (float)fl[1]; p[8] = (float)fl[2];
            p[9] = conf;
        }
        fg |= in;
    }

    // ---- the label rule of the mode (get_flow_samples.py:117-148) ----
    const double *Ti = a.tinv + (size_t)f * 16;
    for (int k = 0; k < slots; ++k) {
        float *p = t1 + (size_t)(t + k * PREP_THREADS) * PREP_COLS1;
        const bool is_fg = fg >> k & 1;
        if (pseudo) {
            p[9] = is_fg ? 1.0f - p[9] : 1.0f;                             // labels: the box flow, or the zeros written above
            continue;
        }
        double fr[3];
        prep_flow(Ti, (double)p[0], (double)p[1], (double)p[2], fr);
        bool moving = false;
        if (is_fg) {                                                       // the float32 label against the float64 rigid flow
            const double d0 = (double)p[6] - fr[0], d1 = (double)p[7] - fr[1], d2 = (double)p[8] - fr[2];
            moving = sqrt((d0 * d0 + d1 * d1) + d2 * d2) > 0.05;
        }
        if (moving) {
            p[9] = 1.0f - p[9];
        } else {
            p[6] = (float)fr[0]; p[7] = (float)fr[1]; p[8] = (float)fr[2];
            p[9] = 1.0f;
        }
    }
    // points beyond CMF_DRAW_MAX_POINTS (the host refuses such frames) keep the background row written above
}

bool filter_args_ok(int C, int W, int H, double zlo, double zhi, const float *scans, const int *scan_off, const double *tcr, const double *proj)
{
    return C >= 5 && W >= 1 && H >= 1 && zlo <= zhi && scans && scan_off && tcr && proj;
}

}  // namespace

extern "C" int cmf_prepare_count(int nscans, int ncols, const float *scans, const int *scan_off, const double *t_camera_radar,
                                 const double *projection, int calib_per_scan, int width, int height, double zlo, double zhi,
                                 int *keep, int *uv, int *count, void *stream)
{
    CMF_CHECK_ARG(nscans >= 1 && filter_args_ok(ncols, width, height, zlo, zhi, scans, scan_off, t_camera_radar, projection));
    CMF_CHECK_ARG(keep && uv && count);
    CountArgs a{{ncols, calib_per_scan != 0, width, height, zlo, zhi, scans, scan_off, t_camera_radar, projection}, keep, uv, count};
    hipLaunchKernelGGL(prepare_count_kernel, dim3(nscans), dim3(PREP_THREADS), 0, (hipStream_t)stream, a);
    return cmf_launch_status();
}

extern "C" int cmf_prepare_scans(int nscans, int ncols, int nmax, const float *scans, const int *scan_off, const double *t_camera_radar,
                                 const double *projection, int calib_per_scan, int width, int height, double zlo, double zhi,
                                 float *pc, float *ft, int *n, void *stream)
{
    CMF_CHECK_ARG(nscans >= 1 && filter_args_ok(ncols, width, height, zlo, zhi, scans, scan_off, t_camera_radar, projection));
    CMF_CHECK_ARG(nmax >= 1 && nmax <= CMF_DRAW_MAX_NPOINTS && pc && ft && n);
    ScansArgs a{{ncols, calib_per_scan != 0, width, height, zlo, zhi, scans, scan_off, t_camera_radar, projection}, nmax, pc, ft, n};
    hipLaunchKernelGGL(prepare_scans_kernel, dim3(nscans), dim3(PREP_THREADS), 0, (hipStream_t)stream, a);
    return cmf_launch_status();
}

extern "C" int cmf_prepare_pairs(int npairs, int ncols, const float *scans, const int *scan_off, const int *keep, const int *uv,
                                 const int *pairs, const int *off1, const int *off2, const double *t_inv, const double *boxes,
                                 const int *box_off, int mode, const float *const *flow, int width, int height,
                                 float *tab1, float *tab2, void *stream)
{
    CMF_CHECK_ARG(npairs >= 1 && ncols >= 5 && width >= 1 && height >= 1);
    CMF_CHECK_ARG(mode == CMF_PREP_MODE_GT || mode == CMF_PREP_MODE_PSEUDO);
    CMF_CHECK_ARG(scans && scan_off && keep && uv && pairs && off1 && off2 && t_inv && boxes && box_off && tab1 && tab2);
    PairsArgs a{npairs, ncols, mode, width, height, scans, scan_off, keep, uv, pairs, off1, off2, t_inv, boxes, box_off, flow, tab1, tab2};
    hipLaunchKernelGGL(prepare_pairs_kernel, dim3(npairs), dim3(PREP_THREADS), 0, (hipStream_t)stream, a);
    return cmf_launch_status();
}
