// A test run's results as bird's-eye-view images (cmflow_amd/vis.py) -- the reference's `--vis` branch
// (main_util.py:170-172; utils/vis_util.py visulize_result_2D_pre / visulize_result_2D_seg_pre with utils/vis_ops.py) without its
// per-frame copies to the host and without matplotlib.
//   cmf_vis_point_colors: one RGB triple and one "drawn" byte per point of the selected frames, float64 from the float32 inputs;
//   cmf_vis_render_bev:   hard discs in index order (the last drawn point over a pixel wins) plus the range / bearing guides, as a
//                         DEFINITION in float32 that uses + - * and compares only.
// Both are restated in numpy, bit for bit (tests/vis_ref.py): no contraction anywhere in this file.
#include "frame_tables.h"

#pragma clang fp contract(off)

namespace {

// The Middlebury wheel (Baker et al., ICCV 2007): 55 entries, segments RY 15 | YG 6 | GC 4 | CB 11 | BM 13 | MR 6; inside a segment of
// length L the moving channel is floor(255 k / L) (rising) or 255 - floor(255 k / L) (falling), k = 0 .. L-1.
constexpr int WHEEL_N = 55;
__device__ const unsigned char WHEEL[WHEEL_N][3] = {
    {255, 0, 0}, {255, 17, 0}, {255, 34, 0}, {255, 51, 0}, {255, 68, 0}, {255, 85, 0}, {255, 102, 0}, {255, 119, 0}, {255, 136, 0},
    {255, 153, 0}, {255, 170, 0}, {255, 187, 0}, {255, 204, 0}, {255, 221, 0}, {255, 238, 0},
    {255, 255, 0}, {213, 255, 0}, {170, 255, 0}, {128, 255, 0}, {85, 255, 0}, {43, 255, 0},
    {0, 255, 0}, {0, 255, 63}, {0, 255, 127}, {0, 255, 191},
    {0, 255, 255}, {0, 232, 255}, {0, 209, 255}, {0, 186, 255}, {0, 163, 255}, {0, 140, 255}, {0, 116, 255}, {0, 93, 255}, {0, 70, 255},
    {0, 47, 255}, {0, 24, 255},
    {0, 0, 255}, {19, 0, 255}, {39, 0, 255}, {58, 0, 255}, {78, 0, 255}, {98, 0, 255}, {117, 0, 255}, {137, 0, 255}, {156, 0, 255},
    {176, 0, 255}, {196, 0, 255}, {215, 0, 255}, {235, 0, 255},
    {255, 0, 255}, {255, 0, 213}, {255, 0, 170}, {255, 0, 128}, {255, 0, 85}, {255, 0, 43}};

constexpr double VIS_PI = 3.141592653589793;                               // numpy's np.pi
constexpr unsigned TOMATO = 255u | (99u << 8) | (71u << 16), ROYAL_BLUE = 65u | (105u << 8) | (225u << 16);
constexpr unsigned BACKGROUND = 80u | (80u << 8) | (80u << 16), WHITE = 255u | (255u << 8) | (255u << 16);

struct ColorArgs {
    int nsel, F, layer, ld_tab;
    long long total;
    const long long *frames;
    const int *off1;
    const float *flow, *tab1;
    const unsigned char *mask;
    unsigned char *colors, *drawn;
};

// The frame of selection slot `s` and its rows [start, start + n) of the store (frame_tables.h: a bad id is clamped, offsets that do not
// describe the store give n = 0).
__device__ __forceinline__ void vis_frame_rows(const long long *frames, const int *off1, int F, long long total, int s, long long &start, int &n)
{
    long long rows;
    ft_frame_rows(off1, ft_selected_frame(frames, s, F), total, start, rows);
    n = (int)rows;                                                         // off1 is int32: rows <= INT_MAX
}

// floor(255 col) as a byte: col lies in [0, 1] for every finite input; anything else (a NaN flow) becomes 0.
__device__ __forceinline__ unsigned vis_level(double col)
{
    const double q = floor(255.0 * col);
    return (q >= 0.0 && q <= 255.0) ? (unsigned)(int)q : 0u;
}

// vis_ops.flow_xy_to_colors for one point, (u, v) as that function takes them: every operation in float64, rounded on its own, in
// the reference's order.  k0 is clamped to the table BEFORE it is used, so no input can index outside it.
__device__ unsigned vis_wheel_color(double u, double v)
{
    const double rad = sqrt(u * u + v * v);
    const double a = atan2(-v, -u) / VIS_PI;
    const double fk = (a + 1.0) / 2.0 * (double)(WHEEL_N - 1);
    const double fl = floor(fk);
    const int k0 = (fl >= 0.0 && fl <= (double)(WHEEL_N - 1)) ? (int)fl : 0;
    const int k1 = k0 + 1 == WHEEL_N ? 0 : k0 + 1;
    const double f = fk - (double)k0;
    unsigned out = 0;
    for (int ch = 0; ch < 3; ++ch) {
        const double col0 = (double)WHEEL[k0][ch] / 255.0, col1 = (double)WHEEL[k1][ch] / 255.0;
        double col = (1.0 - f) * col0 + f * col1;
        if (rad <= 1.0) col = 1.0 - rad * (1.0 - col);
        else col = col * 0.75;
        out |= vis_level(col) << (8 * ch);
    }
    return out;
}

// One wavefront per selected frame, lane-strided over its points.  Layers 0 / 1 first take the maximum of sqrt(fx^2 + fy^2) over
// the frame's PREDICTED flow (max is order-independent: any reduction order is exact), then colour the predicted (0) or the label (1)
// flow normalised by it; layers 2 / 3 colour by the predicted mask byte or the split's mask column.
__global__ __launch_bounds__(CMF_WAVE) void vis_point_colors_kernel(const ColorArgs a)
{
    const int lane = threadIdx.x;
    long long start;
    int n;
    vis_frame_rows(a.frames, a.off1, a.F, a.total, blockIdx.x, start, n);
    double denom = 0.0;
    if (a.layer <= CMF_VIS_FLOW_GT) {
        double rad_max = 0.0;                                              // radii are >= 0, so 0 is the identity of their max
        for (int i = lane; i < n; i += CMF_WAVE) {
            const float *q = a.flow + 3 * (size_t)(start + i);
            const double fx = (double)q[0], fy = (double)q[1];
            rad_max = fmax(rad_max, sqrt(fx * fx + fy * fy));
        }
        for (int off = 32; off > 0; off >>= 1) rad_max = fmax(rad_max, __shfl_xor(rad_max, off, CMF_WAVE));
        denom = rad_max + 1e-5;
    }
    for (int i = lane; i < n; i += CMF_WAVE) {
        const size_t row = (size_t)(start + i);
        unsigned c = 0, draw = 1;
        if (a.layer <= CMF_VIS_FLOW_GT) {
            const float *q = a.layer == CMF_VIS_FLOW ? a.flow + 3 * row : a.tab1 + (size_t)a.ld_tab * row + 6;
            const double x = (double)q[0] / denom, y = (double)q[1] / denom;
            c = vis_wheel_color(x, -y);                                    // vis_util.py:63: flow_xy_to_colors(x_flow, -y_flow)
        } else if (a.layer == CMF_VIS_SEG) {
            c = a.mask[row] ? ROYAL_BLUE : TOMATO;
        } else {
            const float m = a.tab1[(size_t)a.ld_tab * row + 9];
            draw = (m == 0.0f || m == 1.0f) ? 1u : 0u;                     // vis_util.py:139-140: mask == 0, mask == 1, nothing else
            c = m == 0.0f ? TOMATO : m == 1.0f ? ROYAL_BLUE : 0u;
        }
        a.colors[3 * row] = (unsigned char)(c & 255u);
        a.colors[3 * row + 1] = (unsigned char)((c >> 8) & 255u);
        a.colors[3 * row + 2] = (unsigned char)(c >> 16);
        a.drawn[row] = (unsigned char)draw;
    }
}

constexpr int TILE = 16, RENDER_THREADS = TILE * TILE;

struct RenderArgs {
    int nsel, F, W, H, ld_xyz, guides;
    long long total;
    const long long *frames;
    const int *off1;
    const float *xyz;
    const unsigned char *colors, *drawn;
    float x0, y1, s, inv_s, half, radius, r2;
    unsigned char *out;
};

// tan(theta) and sqrt(1 + tan(theta)^2) of the bearing lines at 0, +-5, +-10, +-15 degrees, as float literals (tests/vis_ref.py holds
// the same table)
__device__ const float BEARING[7][2] = {{0.0f, 1.0f}, {0.0874886662f, 1.00381982f}, {-0.0874886662f, 1.00381982f},
                                        {0.176326975f, 1.01542664f}, {-0.176326975f, 1.01542664f},
                                        {0.267949194f, 1.03527617f}, {-0.267949194f, 1.03527617f}};

// The guides at the pixel centre (x, y) in metres, h = half a pixel in metres: range rings at 10 .. 50 m,
// (r-h)^2 <= x^2 + y^2 <= (r+h)^2 with x >= 0 and |y| <= 10 (the 10 m ring) or 12.5; bearing lines |y - t x| <= h k_t, 0 <= x <= 60.
__device__ bool vis_on_guide(float x, float y, float h)
{
    const float q = x * x + y * y, ay = fabsf(y);
    bool on = false;
    for (int k = 1; k <= 5; ++k) {
        const float r = 10.0f * (float)k, lo = r - h, hi = r + h;
        on |= x >= 0.0f && ay <= (k == 1 ? 10.0f : 12.5f) && lo * lo <= q && q <= hi * hi;
    }
    for (int k = 0; k < 7; ++k)
        on |= x >= 0.0f && x <= 60.0f && fabsf(y - BEARING[k][0] * x) <= h * BEARING[k][1];
    return on;
}

// One workgroup per (16 x 16-pixel tile, selected frame); thread t owns pixel (t >> 4, t & 15) of the tile.  The frame's points pass
// through LDS in chunks of 256: thread t tests point base + t against the tile's box grown by radius + 1 pixels (a superset of the
// points that can cover a pixel of the tile: it decides nothing), a ballot per wave and the four waves' counts place the survivors
// in LDS IN INDEX ORDER, and every thread walks them in that order -- the last one covering its pixel stays.  No atomics, no race:
// a pixel is written once, by its own thread, through the tile's LDS image (whole dwords where the canvas rows are dword-aligned).
__global__ __launch_bounds__(RENDER_THREADS) void vis_render_bev_kernel(const RenderArgs a)
{
    __shared__ float s_u[RENDER_THREADS], s_v[RENDER_THREADS];
    __shared__ unsigned s_c[RENDER_THREADS];
    __shared__ int s_cnt[RENDER_THREADS / CMF_WAVE];
    __shared__ unsigned s_img[TILE * TILE * 3 / 4];
    const int tid = threadIdx.x, lane = tid & (CMF_WAVE - 1), wave = tid / CMF_WAVE;
    const int c0 = blockIdx.x * TILE, r0 = blockIdx.y * TILE;
    const int c = c0 + (tid & (TILE - 1)), r = r0 + (tid >> 4);
    const float cx = (float)c + 0.5f, cy = (float)r + 0.5f;
    const float grow = a.radius + 1.0f;
    const float bx0 = (float)c0 - grow, bx1 = (float)(c0 + TILE) + grow, by0 = (float)r0 - grow, by1 = (float)(r0 + TILE) + grow;
    long long start;
    int n;
    vis_frame_rows(a.frames, a.off1, a.F, a.total, blockIdx.z, start, n);
    unsigned best = BACKGROUND;
    for (int base = 0; base < n; base += RENDER_THREADS) {
        const int i = base + tid;
        bool keep = false;
        float pu = 0.0f, pv = 0.0f;
        unsigned col = 0;
        if (i < n) {
            const size_t row = (size_t)(start + i);
            if (a.drawn[row]) {
                const float *p = a.xyz + (size_t)a.ld_xyz * row;
                pu = (p[0] - a.x0) * a.inv_s;
                pv = (a.y1 - p[1]) * a.inv_s;
                keep = pu >= bx0 && pu <= bx1 && pv >= by0 && pv <= by1;   // false for a NaN coordinate
                col = (unsigned)a.colors[3 * row] | ((unsigned)a.colors[3 * row + 1] << 8) | ((unsigned)a.colors[3 * row + 2] << 16);
            }
        }
        const unsigned long long hits = __ballot(keep);
        const int lower = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(hits >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hits, 0u));
        if (lane == 0) s_cnt[wave] = __popcll(hits);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < RENDER_THREADS / CMF_WAVE; ++w) {
            before += w < wave ? s_cnt[w] : 0;
            all += s_cnt[w];
        }
        if (keep) {
            s_u[before + lower] = pu;
            s_v[before + lower] = pv;
            s_c[before + lower] = col;
        }
        __syncthreads();
        for (int j = 0; j < all; ++j) {
            const float dx = cx - s_u[j], dy = cy - s_v[j];
            if (dx * dx + dy * dy <= a.r2) best = s_c[j];
        }
        __syncthreads();                                                   // the next chunk overwrites s_cnt and the lists
    }
    if (a.guides && vis_on_guide(a.x0 + cx * a.s, a.y1 - cy * a.s, a.half)) best = WHITE;
    unsigned char *img = reinterpret_cast<unsigned char *>(s_img);
    img[3 * tid] = (unsigned char)(best & 255u);
    img[3 * tid + 1] = (unsigned char)((best >> 8) & 255u);
    img[3 * tid + 2] = (unsigned char)(best >> 16);
    __syncthreads();
    unsigned char *out = a.out + (size_t)blockIdx.z * a.H * a.W * 3;
    if ((a.W & 3) == 0 && c0 + TILE <= a.W) {                              // rows start on dwords: 12 dwords per tile row
        constexpr int DW = TILE * 3 / 4;
        if (tid < TILE * DW) {
            const int row = tid / DW, k = tid % DW;
            if (r0 + row < a.H)
                reinterpret_cast<unsigned *>(out + ((size_t)(r0 + row) * a.W + c0) * 3)[k] = s_img[row * DW + k];
        }
    } else if (c < a.W && r < a.H) {
        unsigned char *o = out + ((size_t)r * a.W + c) * 3;
        o[0] = img[3 * tid]; o[1] = img[3 * tid + 1]; o[2] = img[3 * tid + 2];
    }
}

}  // namespace

extern "C" int cmf_vis_point_colors(int nsel, int nframes, const long long *frames, const int *off1, long long total, int layer,
                                    const float *flow, const float *tab1, int ld_tab, const unsigned char *mask,
                                    unsigned char *colors, unsigned char *drawn, void *stream)
{
    CMF_CHECK_ARG(nsel >= 0 && nframes >= 1 && total >= 0 && layer >= CMF_VIS_FLOW && layer <= CMF_VIS_SEG_GT);
    if (nsel == 0) return 0;
    CMF_CHECK_ARG(off1 && colors && drawn);
    CMF_CHECK_ARG(frames || nsel <= nframes);
    CMF_CHECK_ARG(layer > CMF_VIS_FLOW_GT || flow);
    CMF_CHECK_ARG((layer != CMF_VIS_FLOW_GT && layer != CMF_VIS_SEG_GT) || (tab1 && ld_tab >= 10));
    CMF_CHECK_ARG(layer != CMF_VIS_SEG || mask);
    ColorArgs a{nsel, nframes, layer, ld_tab, total, frames, off1, flow, tab1, mask, colors, drawn};
    hipLaunchKernelGGL(vis_point_colors_kernel, dim3(nsel), dim3(CMF_WAVE), 0, (hipStream_t)stream, a);
    return cmf_launch_status();
}

extern "C" int cmf_vis_render_bev(int nsel, int nframes, const long long *frames, const int *off1, long long total, const float *xyz,
                                  int ld_xyz, const unsigned char *colors, const unsigned char *drawn, int width, int height,
                                  float x0, float y1, float s, float inv_s, float half, float radius, float r2, int guides,
                                  unsigned char *out, void *stream)
{
    CMF_CHECK_ARG(nsel >= 0 && nsel <= 65535 && nframes >= 1 && total >= 0);   // nsel is the grid's z extent
    CMF_CHECK_ARG(width >= 1 && width <= CMF_VIS_MAX_SIDE && height >= 1 && height <= CMF_VIS_MAX_SIDE);
    if (nsel == 0) return 0;
    CMF_CHECK_ARG(off1 && xyz && ld_xyz >= 2 && colors && drawn && out);
    CMF_CHECK_ARG(frames || nsel <= nframes);
    CMF_CHECK_ARG(radius > 0.0f && radius <= (float)CMF_VIS_MAX_SIDE && r2 >= 0.0f && r2 <= (radius + 0.5f) * (radius + 0.5f));
    RenderArgs a{nsel, nframes, width, height, ld_xyz, guides, total, frames, off1, xyz, colors, drawn, x0, y1, s, inv_s, half, radius, r2, out};
    hipLaunchKernelGGL(vis_render_bev_kernel, dim3(cmf_divup(width, TILE), cmf_divup(height, TILE), nsel), dim3(RENDER_THREADS), 0,
                       (hipStream_t)stream, a);
    return cmf_launch_status();
}
