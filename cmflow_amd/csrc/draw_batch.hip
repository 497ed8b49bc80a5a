// cmf_draw_batch: one training batch drawn from a split that lives on the device (cmflow_amd/dataset.py DeviceSplit) -- frame
// choice, the reference's per-frame resampling to `npoints` (dataset/vod.py:95-121 sample_points = dataset._resample) and the model's
// layout (main_util.py:21-36 extract_data_info) in ONE launch.  One workgroup per (slot, cloud).
//
// Sampling contract (include/cmflow_hip.h, DESIGN.md "Device-resident split"): Philox4x32-10, keyed per call from (seed, draw),
// counter (slot0 + slot, cloud, i, 0), word 0 of the output (slot0 = 0 for cmf_draw_batch; cmf_draw_batch_at: the local batch is
// slots slot0 .. slot0 + B - 1 of a larger one, every index into frames and outputs stays local).
//   n <  N: points 0 .. n-1 in order, then N - n independent draws mulhi(u32, n)                          -- no sort;
//   n >= N: point i carries the 64-bit key (u32 << 32) | i; the keys go to LDS, padded with maximal keys to the next power of two,
//           a bitonic sort puts them in ascending order and the low words of the first N are the draw (a uniformly random
//           N-subset in uniformly random order; keys are distinct by construction).
// The chosen indices stay in LDS; the gather then runs output tensor by output tensor with consecutive lanes on consecutive
// addresses of the output (the reads are 4-byte picks from 56- / 24-byte rows of a table that sits in L2).
//
// cmf_draw_frames (below, same tables): the frames themselves, whole and unsampled, padded to a ragged batch.
#include "cmf_common.h"
#include "philox.h"
#include "../../include/cmflow_hip.h"

namespace {

constexpr int DRAW_COLS1 = 14, DRAW_COLS2 = 6;
constexpr int DRAW_THREADS_SMALL = 256, DRAW_THREADS_LARGE = 1024;     // the large form from 4096 sort slots on

struct DrawArgs {
    int B, N, F, max_points;
    int slot0;                                                             // counter word 0 of local slot s is slot0 + s
    const float *tab1, *tab2;
    const int *off1, *off2;
    const float *trans, *interval;
    const int *frames;
    uint32_t k0, k1;
    float *pc1, *pc2, *ft1, *ft2, *gt_trans, *flow_label, *fg_mask, *interval_out, *radar_u, *radar_v, *opt_flow;
    int *idx1, *idx2;
};

__global__ __launch_bounds__(DRAW_THREADS_LARGE) void draw_batch_kernel(const DrawArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long draw_keys[];     // [P] sort keys, or [N] ints when n < N
    int *sel = reinterpret_cast<int *>(draw_keys);
    const int slot = blockIdx.x, cloud = blockIdx.y, t = threadIdx.x, nt = blockDim.x;
    const int N = a.N;
    const uint32_t cslot = (uint32_t)(a.slot0 + slot);                     // the generator's slot; every index below uses the local one
    const int f = min(max(a.frames[slot], 0), a.F - 1);                    // a bad id gives wrong data, not a wild access
    const int *off = cloud ? a.off2 : a.off1;
    const long long start = off[f];
    const int n = min(max(off[f + 1] - off[f], 1), a.max_points);          // the LDS was sized for max_points
    int sh;                                                                // the draw of output j is sel[j << sh]
    if (n < N) {
        sh = 0;
        for (int j = t; j < N; j += nt)
            sel[j] = j < n ? j : (int)draw_mulhi(philox4x32_10(cslot, cloud, j - n, 0u, a.k0, a.k1).x, (uint32_t)n);
        __syncthreads();
    } else {
        sh = 1;                                                            // low word of key j (little endian)
        int P = 1;
        while (P < n) P <<= 1;
        for (int i = t; i < P; i += nt)
            draw_keys[i] = i < n ? ((unsigned long long)philox4x32_10(cslot, cloud, i, 0u, a.k0, a.k1).x << 32) | (unsigned)i : ~0ull;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int h = t; h < (P >> 1); h += nt) {
                    const int lo = ((h & ~(j - 1)) << 1) | (h & (j - 1)), hi = lo | j;
                    const unsigned long long x = draw_keys[lo], y = draw_keys[hi];
                    if ((x > y) == ((lo & k) == 0)) {
                        draw_keys[lo] = y;
                        draw_keys[hi] = x;
                    }
                }
                __syncthreads();
            }
    }
    const size_t sN = (size_t)slot * N;
    if (cloud == 0) {
        const float *tab = a.tab1 + (size_t)start * DRAW_COLS1;
        for (int e = t; e < 3 * N; e += nt) {                              // (B,3,N): coordinates and features
            const int c = e / N, j = e - c * N;
            const float *row = tab + (size_t)sel[j << sh] * DRAW_COLS1;
            a.pc1[3 * sN + e] = row[c];
            a.ft1[3 * sN + e] = row[3 + c];
        }
        for (int e = t; e < 3 * N; e += nt) {                              // (B,N,3): labels
            const int j = e / 3, c = e - 3 * j;
            a.flow_label[3 * sN + e] = tab[(size_t)sel[j << sh] * DRAW_COLS1 + 6 + c];
        }
        for (int e = t; e < 2 * N; e += nt)                                // (B,N,2): optical flow
            a.opt_flow[2 * sN + e] = tab[(size_t)sel[(e >> 1) << sh] * DRAW_COLS1 + 12 + (e & 1)];
        for (int j = t; j < N; j += nt) {                                  // (B,N)
            const int i = sel[j << sh];
            const float *row = tab + (size_t)i * DRAW_COLS1;
            a.fg_mask[sN + j] = row[9];
            a.radar_u[sN + j] = row[10];
            a.radar_v[sN + j] = row[11];
            a.idx1[sN + j] = i;
        }
        for (int e = t; e < 16; e += nt) a.gt_trans[(size_t)slot * 16 + e] = a.trans[(size_t)f * 16 + e];
        if (t == 0) a.interval_out[slot] = a.interval[f];
    } else {
        const float *tab = a.tab2 + (size_t)start * DRAW_COLS2;
        for (int e = t; e < 3 * N; e += nt) {
            const int c = e / N, j = e - c * N;
            const float *row = tab + (size_t)sel[j << sh] * DRAW_COLS2;
            a.pc2[3 * sN + e] = row[c];
            a.ft2[3 * sN + e] = row[3 + c];
        }
        for (int j = t; j < N; j += nt) a.idx2[sN + j] = sel[j << sh];
    }
}

// cmf_draw_frames: whole frames as a ragged batch (dataset.collate_ragged's padding rule, extract_data_info_ragged's layout).  One
// workgroup per (chunk of FRAMES_CHUNK positions, cloud, slot); lane t holds position p0 + t and reads table row p0 + t (row 0 from
// the frame's count on), so a wave reads 64 consecutive 56- / 24-byte rows -- whole cache lines, every byte of which one of the
// loops below uses -- and every store runs over consecutive addresses of its output tensor.
constexpr int FRAMES_CHUNK = 256;

struct FramesArgs {
    int B, N1, N2, F;
    const float *tab1, *tab2;
    const int *off1, *off2;
    const float *trans, *interval;
    const int *frames;
    float *pc1, *pc2, *ft1, *ft2, *gt_trans, *flow_label, *fg_mask, *interval_out, *radar_u, *radar_v, *opt_flow;
    int *n1, *n2;
};

__global__ __launch_bounds__(FRAMES_CHUNK) void draw_frames_kernel(const FramesArgs a)
{
    const int chunk = blockIdx.x, cloud = blockIdx.y, slot = blockIdx.z, t = threadIdx.x;
    const int N = cloud ? a.N2 : a.N1;
    const int p0 = chunk * FRAMES_CHUNK;
    if (p0 >= N) return;                                                   // the grid covers the larger of the two clouds
    const int cnt = min(FRAMES_CHUNK, N - p0);                             // positions of this chunk
    const int f = min(max(a.frames[slot], 0), a.F - 1);                    // a bad id gives wrong data, not a wild access
    const int *off = cloud ? a.off2 : a.off1;
    const long long start = off[f];
    const int n = min(max(off[f + 1] - off[f], 1), N);                     // a too-small nmax truncates the frame
    const size_t sN = (size_t)slot * N + p0;                               // the chunk's first position in a (B,N) tensor
    const long long last = max(off[a.F] - 1, 0);                           // an empty frame in the offsets reads a neighbour's row, not past the table
    const auto row_of = [&](int j) { return (size_t)min(start + (p0 + j < n ? p0 + j : 0), last); };
    if (cloud == 0) {
        const float *tab = a.tab1;
        if (t < cnt) {
            const float *row = tab + row_of(t) * DRAW_COLS1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {                                  // (B,3,N): coordinates and features
                const size_t o = ((size_t)slot * 3 + c) * N + p0 + t;
                a.pc1[o] = row[c];
                a.ft1[o] = row[3 + c];
            }
            a.fg_mask[sN + t] = row[9];                                    // (B,N)
            a.radar_u[sN + t] = row[10];
            a.radar_v[sN + t] = row[11];
        }
        for (int e = t; e < 3 * cnt; e += FRAMES_CHUNK) {                  // (B,N,3): labels
            const int j = e / 3, c = e - 3 * j;
            a.flow_label[3 * sN + e] = tab[row_of(j) * DRAW_COLS1 + 6 + c];
        }
        for (int e = t; e < 2 * cnt; e += FRAMES_CHUNK)                    // (B,N,2): optical flow
            a.opt_flow[2 * sN + e] = tab[row_of(e >> 1) * DRAW_COLS1 + 12 + (e & 1)];
        if (chunk == 0) {
            if (t < 16) a.gt_trans[(size_t)slot * 16 + t] = a.trans[(size_t)f * 16 + t];
            if (t == 0) {
                a.interval_out[slot] = a.interval[f];
                a.n1[slot] = n;
            }
        }
    } else {
        if (t < cnt) {
            const float *row = a.tab2 + row_of(t) * DRAW_COLS2;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const size_t o = ((size_t)slot * 3 + c) * N + p0 + t;
                a.pc2[o] = row[c];
                a.ft2[o] = row[3 + c];
            }
        }
        if (chunk == 0 && t == 0) a.n2[slot] = n;
    }
}

}  // namespace

extern "C" int cmf_draw_batch_at(int slot0, int B, int npoints, int nframes, int max_points, const float *tab1, const float *tab2,
                                 const int *off1, const int *off2, const float *trans, const float *interval, const int *frames,
                                 unsigned long long seed, unsigned long long draw,
                                 float *pc1, float *pc2, float *ft1, float *ft2, float *gt_trans, float *flow_label, float *fg_mask,
                                 float *interval_out, float *radar_u, float *radar_v, float *opt_flow, int *idx1, int *idx2, void *stream)
{
    CMF_CHECK_ARG(slot0 >= 0 && B >= 1 && (long long)slot0 + B <= 2147483647LL);
    CMF_CHECK_ARG(B >= 1 && npoints >= 1 && npoints <= CMF_DRAW_MAX_NPOINTS && nframes >= 1);
    CMF_CHECK_ARG(max_points >= 1 && max_points <= CMF_DRAW_MAX_POINTS);
    CMF_CHECK_ARG(tab1 && tab2 && off1 && off2 && trans && interval && frames);
    CMF_CHECK_ARG(pc1 && pc2 && ft1 && ft2 && gt_trans && flow_label && fg_mask && interval_out && radar_u && radar_v && opt_flow && idx1 && idx2);
    int P = 1;
    while (P < max_points) P <<= 1;
    const size_t lds = std::max((size_t)P * 8, (size_t)npoints * 4);       // <= 128 KiB by the two limits above
    static CmfPerDevice attr_set;
    int attr_dev;
    if (attr_set.need(attr_dev)) {
        const hipError_t e = hipFuncSetAttribute((const void *)draw_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 CMF_DRAW_MAX_POINTS * 8);
        if (e != hipSuccess) return (int)e;
        attr_set.done(attr_dev);
    }
    const Philox key = philox_call_key(seed, draw);
    DrawArgs a{B, npoints, nframes, max_points, slot0, tab1, tab2, off1, off2, trans, interval, frames, key.x, key.y,
               pc1, pc2, ft1, ft2, gt_trans, flow_label, fg_mask, interval_out, radar_u, radar_v, opt_flow, idx1, idx2};
    const int threads = P >= 4096 ? DRAW_THREADS_LARGE : DRAW_THREADS_SMALL;
    hipLaunchKernelGGL(draw_batch_kernel, dim3(B, 2), dim3(threads), lds, (hipStream_t)stream, a);
    return cmf_launch_status();
}

extern "C" int cmf_draw_batch(int B, int npoints, int nframes, int max_points, const float *tab1, const float *tab2, const int *off1,
                              const int *off2, const float *trans, const float *interval, const int *frames,
                              unsigned long long seed, unsigned long long draw,
                              float *pc1, float *pc2, float *ft1, float *ft2, float *gt_trans, float *flow_label, float *fg_mask,
                              float *interval_out, float *radar_u, float *radar_v, float *opt_flow, int *idx1, int *idx2, void *stream)
{
    return cmf_draw_batch_at(0, B, npoints, nframes, max_points, tab1, tab2, off1, off2, trans, interval, frames, seed, draw,
                             pc1, pc2, ft1, ft2, gt_trans, flow_label, fg_mask, interval_out, radar_u, radar_v, opt_flow, idx1, idx2, stream);
}

extern "C" int cmf_draw_frames(int B, int nmax1, int nmax2, int nframes, const float *tab1, const float *tab2, const int *off1,
                               const int *off2, const float *trans, const float *interval, const int *frames,
                               float *pc1, float *pc2, float *ft1, float *ft2, float *gt_trans, float *flow_label, float *fg_mask,
                               float *interval_out, float *radar_u, float *radar_v, float *opt_flow, int *n1, int *n2, void *stream)
{
    CMF_CHECK_ARG(B >= 1 && B <= 65535 && nframes >= 1);                   // B is the grid's z extent
    CMF_CHECK_ARG(nmax1 >= 1 && nmax1 <= CMF_DRAW_MAX_NPOINTS && nmax2 >= 1 && nmax2 <= CMF_DRAW_MAX_NPOINTS);
    CMF_CHECK_ARG(tab1 && tab2 && off1 && off2 && trans && interval && frames);
    CMF_CHECK_ARG(pc1 && pc2 && ft1 && ft2 && gt_trans && flow_label && fg_mask && interval_out && radar_u && radar_v && opt_flow && n1 && n2);
    FramesArgs a{B, nmax1, nmax2, nframes, tab1, tab2, off1, off2, trans, interval, frames,
                 pc1, pc2, ft1, ft2, gt_trans, flow_label, fg_mask, interval_out, radar_u, radar_v, opt_flow, n1, n2};
    const int chunks = (std::max(nmax1, nmax2) + FRAMES_CHUNK - 1) / FRAMES_CHUNK;
    hipLaunchKernelGGL(draw_frames_kernel, dim3(chunks, 2, B), dim3(FRAMES_CHUNK), 0, (hipStream_t)stream, a);
    return cmf_launch_status();
}
