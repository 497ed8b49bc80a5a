// The frame and clip tables of a test run's analysis chain (vis, accumulate, instances, tracks, objects; DESIGN.md sections 20-24), as
// every kernel of the chain reads them: which frame a block works on and which rows it owns, a clip's bounds and which of its frames
// own their rows, the ranks of a workgroup's flags, and the two pieces of float64 arithmetic the definitions share.  ONE statement of
// each rule: the numpy restatements under tests/ pin every kernel that uses them bit for bit.  Device functions only, no contraction.
#pragma once
#include "cmf_common.h"
#include "../../include/cmflow_hip.h"

#pragma clang fp contract(off)

// ranks of the set flags of a workgroup of WAVES waves, in thread order: -> (flags of lower threads, flags of the workgroup).  A ballot
// per wave and the waves' counts through s_cnt[WAVES]; two barriers, the second because the next scan overwrites s_cnt.  Called by
// every thread.
template <int WAVES>
__device__ __forceinline__ void ft_block_rank(bool flag, int lane, int wave, int *s_cnt, int &before, int &all)
{
    const unsigned long long hits = __ballot(flag);
    const int lower = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(hits >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hits, 0u));
    if (lane == 0) s_cnt[wave] = __popcll(hits);
    __syncthreads();
    before = lower;
    all = 0;
    for (int w = 0; w < WAVES; ++w) {
        before += w < wave ? s_cnt[w] : 0;
        all += s_cnt[w];
    }
    __syncthreads();
}

// ((m0 x + m1 y) + m2 z) + m3, every operation rounded on its own: one row of an affine map
__device__ __forceinline__ double ft_affine(const double *m, double x, double y, double z) { return ((m[0] * x + m[1] * y) + m[2] * z) + m[3]; }

// d = (p + flow) - T p: the displacement a point shows against the ego-motion T (the first three rows of the frame's transform)
__device__ __forceinline__ void ft_own_motion(const double *T, double px, double py, double pz, const float *flow, double d[3])
{
    d[0] = (px + (double)flow[0]) - ft_affine(T, px, py, pz);
    d[1] = (py + (double)flow[1]) - ft_affine(T + 4, px, py, pz);
    d[2] = (pz + (double)flow[2]) - ft_affine(T + 8, px, py, pz);
}

// the frame of selection slot s (frames == NULL: slot s is frame s); a bad id is clamped to 0 .. F-1, so it lands in a wrong frame and
// not outside the tables
__device__ __forceinline__ int ft_selected_frame(const long long *frames, int s, int F)
{
    long long f = frames ? frames[s] : (long long)s;
    f = f < 0 ? 0 : f > F - 1 ? F - 1 : f;
    return (int)f;
}

// the rows [start, start + n) of frame f; offsets that do not describe the tables (outside 0 .. total, or descending) give n = 0
__device__ __forceinline__ void ft_frame_rows(const int *off1, int f, long long total, long long &start, long long &n)
{
    start = off1[f];
    n = (long long)off1[f + 1] - start;
    if (start < 0 || n < 0 || start + n > total) n = 0;
}

// a clip's frames [first, end) clamped to 0 .. F, the row its tables start at, and whether that row lies inside the tables (a clip that
// starts outside them owns no rows)
__device__ __forceinline__ void ft_clip(const int *clips, const int *off1, int clip, int F, long long total, int &first, int &end, long long &base,
                                        bool &clip_ok)
{
    first = clips[2 * clip];
    end = clips[2 * clip + 1];
    first = first < 0 ? 0 : first > F ? F : first;
    end = end < first ? first : end > F ? F : end;
    base = off1[first];
    clip_ok = base >= 0 && base <= total;
}

// one step of the walk over a clip's frames, top = the end of the last frame that owned rows (the clip's base before the first): the
// frame owns its rows [start, stop) iff top <= start <= stop <= total -- in order inside the tables, so the frames' rows are disjoint
// -- and top moves behind them.  -> owns, n = its rows (0 where it owns none)
__device__ __forceinline__ bool ft_clip_frame(bool clip_ok, long long start, long long stop, long long total, long long &top, int &n)
{
    const bool owns = clip_ok && start >= top && stop >= start && stop <= total;
    n = owns ? (int)(stop - start) : 0;
    if (owns) top = stop;
    return owns;
}

// the instances of such a frame: *count clamped to 0 .. min(n, CMF_TRACK_MAX_LIVE), 0 (and *count not read) where it owns no rows
__device__ __forceinline__ int ft_clip_frame_instances(bool owns, const int *count, int n)
{
    int K = owns ? *count : 0;
    K = K < 0 ? 0 : K > n ? n : K;
    return K > CMF_TRACK_MAX_LIVE ? CMF_TRACK_MAX_LIVE : K;
}
