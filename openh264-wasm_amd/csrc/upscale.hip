// upscale.hip -- I420 pictures enlarged on the device (gfx950), as include/h264mi.h defines it (h264mi_i420_upscale_dev,
// h264mi_i420_compose_any_dev, h264mi_speaker_cells, h264mi_enc_encode_composed_any). DESIGN.md §5.7.
//   upscale_kernel : up to H264MI_UPSCALE_PER_LAUNCH enlarging cells per launch -- whole frames (one cell repeated over
//                    n frames), the enlarging cells of a compose_any call, or those of an encoder's composed input
// A cell takes a crop of one source frame to a rectangle of one canvas that is at least as large both ways. Per plane
// (chroma: origin and sizes halved) and per axis, with p the crop's size and q the rectangle's, output index o reads
//   N = (2 o + 1) p - q,  P = floor((16 N + q) / (2 q)),  i = P >> 4,  f = P & 15
// and the taps i - 1 .. i + 2, each clamped to 0 .. p - 1 of the crop, under the weights of phase f (up_weights: the
// Catmull-Rom polynomials in sixteenths scaled to a sum of 8192, or the two bilinear ones). Horizontal first,
// H = (sum Wx p + 16) >> 5, then out = clamp((sum Wy H + 2^20) >> 21, 0, 255): int32 throughout, |sum Wy H| < 2^31.
// The launch scheme is compose_kernel's: the cells and a prefix table of waves per cell travel as kernel arguments, a
// wave finds its cell by a scalar binary search, then plane, strip and segment. A wave owns 64 output columns by
// H264MI_UPSCALE_ROWS output rows of one plane of one cell, a lane per column. A lane computes its column's taps and
// weights once and holds the four horizontally filtered source rows H of the current output row in registers. i grows
// by at most one from an output row to the next (q >= p), so the window slides by one row or stays: an output row
// costs four multiply-adds, and a new source row (four byte loads a lane, two for bilinear) only when i advances. The
// row after the window is loaded one step ahead, so its latency lies under the rows that need no load.
// Bytes are loaded one by one (neighbouring lanes share them when enlarging: a wave's row is 64 p / q + 3 bytes); an
// output row segment is stored as dwords where its first address is a multiple of 4 and the group of four lies inside
// the rectangle, else as bytes (compose's rule, picture_dev.h's seg_put). Nothing is read outside the crop, nothing
// written outside the rectangle. No atomics, no device allocation, no host-to-device copy.
//
// A translation unit and a code object of its own, as quality.hip, scale.hip, compose.hip and overlay.hip are.
// Shrinking cells of a compose_any call go to compose.hip's launch_compose_i420 as they are. The host runtime (capi_enc.inc) reaches this file through the functions
// picture_host.h declares; the checks of a cell list and the cell table of a launch are there too.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include <stdint.h>
#include "../../include/h264mi.h"
#include "picture_host.h"
#include "picture_dev.h"

namespace h264mi {
#define H264MI_UPSCALE_ROWS 32          // output rows per wave
#define H264MI_UPSCALE_MAX_ITEMS (1 << 30)  // waves' worth of work in one launch

typedef PictureCell UpscaleCell;  // a cell as the kernel reads it, 24 bytes (picture_host.h)
struct UpscaleLaunch {
    const uint8_t *src;
    uint8_t *dst;
    size_t sfb, dfb;                              // source frame f: src + f * sfb; canvas c: dst + c * dfb
    int src_w, src_h, cw, ch;
    int ncells, nrep, filter;                     // the cells are repeated nrep times, repetition r on frames src + r, canvas + r
    int first[H264MI_UPSCALE_PER_LAUNCH + 1];     // cell k's waves are first[k] .. first[k + 1] - 1
    UpscaleCell cell[H264MI_UPSCALE_PER_LAUNCH];
};
static_assert(sizeof(UpscaleLaunch) < 2048, "the argument block stays well below 4 KB");

// the four weights of phase f: up_weights, picture_host.h (warp.hip samples under the same ones)
// P of output index o: floor((16 ((2 o + 1) p - q) + q) / (2 q)). The numerator is above -15 q, so 32 q added makes it
// positive (and leaves it below 2^31 for p <= 4096, q <= 8192); the quotient is then 16 too large
__host__ __device__ static inline int up_phase(int o, int p, int q) {
    const uint32_t num = (uint32_t)(16 * ((2 * o + 1) * p - q) + 33 * q);
    return (int)(num / (uint32_t)(2 * q)) - 16;
}

// waves across and down a qw x qh rectangle of one plane
__host__ __device__ static inline int upscale_nstrip(int qw) { return (qw + 63) / 64; }
__host__ __device__ static inline int upscale_nseg(int qh) { return (qh + H264MI_UPSCALE_ROWS - 1) / H264MI_UPSCALE_ROWS; }

struct UpTaps { uint32_t t[4]; };
// a lane's four taps of one plane row (two for bilinear, whose outer weights are 0)
PICDEV UpTaps up_load(const uint8_t *row, const int *xi, bool cubic) {
    UpTaps r;
    r.t[1] = row[xi[1]];
    r.t[2] = row[xi[2]];
    r.t[0] = cubic ? row[xi[0]] : 0u;
    r.t[3] = cubic ? row[xi[3]] : 0u;
    return r;
}
PICDEV int up_hfilter(const UpTaps &r, const int *wx) {
    const int h = wx[0] * (int)r.t[0] + wx[1] * (int)r.t[1] + wx[2] * (int)r.t[2] + wx[3] * (int)r.t[3];
    return (h + 16) >> 5;  // 8 fractional bits, -8160 .. 73440
}

__global__ __launch_bounds__(256) void upscale_kernel(UpscaleLaunch a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // scalar: what follows from it is per wave
    const int per = a.first[a.ncells], items = per * a.nrep;
    const bool cubic = a.filter == H264MI_FILTER_BICUBIC;
    for (int it0 = (int)blockIdx.x * 4 + wave; it0 < items; it0 += (int)gridDim.x * 4) {
        const int rep = a.nrep > 1 ? it0 / per : 0, it = it0 - rep * per;
        int lo_c = 0, hi_c = a.ncells;  // first[lo_c] <= it < first[hi_c]
        while (hi_c - lo_c > 1) {
            const int mid_c = (lo_c + hi_c) >> 1;
            if (a.first[mid_c] <= it) lo_c = mid_c; else hi_c = mid_c;
        }
        const UpscaleCell c = a.cell[lo_c];
        int k = it - a.first[lo_c];  // the wave's index within the cell
        const int lw = upscale_nstrip(c.dw) * upscale_nseg(c.dh), cwv = upscale_nstrip(c.dw >> 1) * upscale_nseg(c.dh >> 1);
        int p = 0;
        if (k >= lw) { k -= lw; p = 1; if (k >= cwv) { k -= cwv; p = 2; } }
        const int sh1 = p != 0;  // chroma: every size and origin halved
        const int pw = c.sw >> sh1, ph = c.sh >> sh1, qw = c.dw >> sh1, qh = c.dh >> sh1;
        const int spitch = a.src_w >> sh1, dpitch = a.cw >> sh1;
        const size_t sy_b = (size_t)a.src_w * a.src_h, sc_b = (size_t)(a.src_w >> 1) * (a.src_h >> 1);
        const size_t dy_b = (size_t)a.cw * a.ch, dc_b = (size_t)(a.cw >> 1) * (a.ch >> 1);
        // the crop's first sample in the source plane; the rectangle's first sample
        const uint8_t *S = a.src + (size_t)(c.src + rep) * a.sfb + (p == 0 ? 0 : p == 1 ? sy_b : sy_b + sc_b) +
                           (size_t)(c.sy >> sh1) * spitch + (c.sx >> sh1);
        uint8_t *D = a.dst + (size_t)(c.canvas + rep) * a.dfb + (p == 0 ? 0 : p == 1 ? dy_b : dy_b + dc_b) + (size_t)(c.dy >> sh1) * dpitch +
                     (c.dx >> sh1);
        const int nstrip = upscale_nstrip(qw);
        const int strip = k % nstrip, seg = k / nstrip;
        const int ox = strip * 64 + lane;
        // the lane's taps, columns of the crop, and their weights; a lane beyond the rectangle takes the last column's
        int xi[4], wx[4];
        {
            const int P = up_phase(min(ox, qw - 1), pw, qw), i = P >> 4;
            up_weights(P & 15, cubic, wx);
#pragma unroll
            for (int t = 0; t < 4; t++) xi[t] = min(max(i - 1 + t, 0), pw - 1);
        }
        const int oy0 = seg * H264MI_UPSCALE_ROWS, oy1 = min(oy0 + H264MI_UPSCALE_ROWS, qh);
        // the window: H[t] is crop row clamp(cur - 1 + t) filtered horizontally; nxt holds the taps of row clamp(cur + 3)
        int cur = up_phase(oy0, ph, qh) >> 4;
        int H[4];
#pragma unroll
        for (int t = 0; t < 4; t++) H[t] = up_hfilter(up_load(S + (size_t)min(max(cur - 1 + t, 0), ph - 1) * spitch, xi, cubic), wx);
        UpTaps nxt = up_load(S + (size_t)min(max(cur + 3, 0), ph - 1) * spitch, xi, cubic);
        for (int oy = oy0; oy < oy1; oy++) {
            const int P = up_phase(oy, ph, qh), i = P >> 4;  // the same in every lane; i is cur or cur + 1
            if (i != cur) {
                cur = i;
                H[0] = H[1]; H[1] = H[2]; H[2] = H[3];
                H[3] = up_hfilter(nxt, wx);
                nxt = up_load(S + (size_t)min(max(cur + 3, 0), ph - 1) * spitch, xi, cubic);
            }
            int wy[4];
            up_weights(P & 15, cubic, wy);
            const int acc = wy[0] * H[0] + wy[1] * H[1] + wy[2] * H[2] + wy[3] * H[3];
            const uint32_t v = (uint32_t)min(max((acc + (1 << 20)) >> 21, 0), 255);
            seg_put(D + (size_t)oy * dpitch + strip * 64, lane, qw - strip * 64, v);  // from the strip's first sample of the row
        }
    }
}

static int upscale_cell_waves(int dw, int dh) {  // at most 128 * 256 + 2 * 64 * 128 waves a cell
    return upscale_nstrip(dw) * upscale_nseg(dh) + 2 * upscale_nstrip(dw / 2) * upscale_nseg(dh / 2);
}

// arguments of a whole-frame upscale call, everything but the pointers' values
bool upscale_args_ok(int dw, int dh, int sw, int sh, int n, int filter) {
    return n > 0 && filter_ok(filter) && sides_ok(dw, dh, sw, sh) && dw >= sw && dh >= sh;
}
// n tight sw x sh I420 frames at src to n tight dw x dh frames at dst; arguments as upscale_args_ok accepts them. One
// cell, the whole frame, repeated over the frames; as many frames to a launch as keep its wave count below 2^30
int launch_upscale_i420(uint8_t *dst, int dw, int dh, const uint8_t *src, int sw, int sh, int n, int filter, hipStream_t s) {
    const h264mi_cell whole{0, 0, 0, 0, sw, sh, 0, 0, dw, dh};
    UpscaleLaunch a{};
    a.sfb = i420_bytes(sw, sh); a.dfb = i420_bytes(dw, dh);
    a.src_w = sw; a.src_h = sh; a.cw = dw; a.ch = dh;
    a.filter = filter;
    a.ncells = fill_cell_table(a.cell, a.first, &whole, 1, upscale_cell_waves);
    const int chunk = H264MI_UPSCALE_MAX_ITEMS / a.first[1];
    (void)hipGetLastError();
    for (int f0 = 0; f0 < n; f0 += chunk) {
        a.nrep = std::min(n - f0, chunk);
        a.src = src + (size_t)f0 * a.sfb;
        a.dst = dst + (size_t)f0 * a.dfb;
        hipLaunchKernelGGL(upscale_kernel, dim3(launch_blocks((long long)a.first[1] * a.nrep)), dim3(256), 0, s, a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// enlarging cells into the canvases at dst, H264MI_UPSCALE_PER_LAUNCH to a launch
static int launch_upscale_cells(uint8_t *dst, int cw, int ch, const uint8_t *src, int src_w, int src_h, const h264mi_cell *cells, int ncells,
                                int filter, hipStream_t s) {
    UpscaleLaunch a{};
    a.src = src; a.dst = dst; a.sfb = i420_bytes(src_w, src_h); a.dfb = i420_bytes(cw, ch);
    a.src_w = src_w; a.src_h = src_h; a.cw = cw; a.ch = ch;
    a.nrep = 1; a.filter = filter;
    (void)hipGetLastError();
    for (int k0 = 0; k0 < ncells; k0 += H264MI_UPSCALE_PER_LAUNCH) {
        a.ncells = fill_cell_table(a.cell, a.first, cells + k0, std::min(ncells - k0, H264MI_UPSCALE_PER_LAUNCH), upscale_cell_waves);
        hipLaunchKernelGGL(upscale_kernel, dim3(launch_blocks(a.first[a.ncells])), dim3(256), 0, s, a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// cells of both kinds (as cells_ok accepts them with enlarging) in list order: the shrinking ones through compose.hip
// as they are, then the enlarging ones. The cells are disjoint, so the order of the two does not matter
int launch_compose_any_i420(uint8_t *dst, int cw, int ch, const uint8_t *src, int src_w, int src_h, const h264mi_cell *cells, int ncells,
                            int filter, hipStream_t s) {
    std::vector<h264mi_cell> shrink, enlarge;
    for (int k = 0; k < ncells; k++) (cell_kind(cells[k]) == 0 ? shrink : enlarge).push_back(cells[k]);
    if (!shrink.empty() && launch_compose_i420(dst, cw, ch, src, src_w, src_h, shrink.data(), (int)shrink.size(), s) != 0) return -1;
    if (!enlarge.empty() && launch_upscale_cells(dst, cw, ch, src, src_w, src_h, enlarge.data(), (int)enlarge.size(), filter, s) != 0) return -1;
    return 0;
}

// the active-speaker layout of include/h264mi.h (h264mi_speaker_cells): host only, integers, floor divisions
int speaker_cells(h264mi_cell *out, int cap, int n, int speaker, int src_w, int src_h, int cw, int ch) {
    if (!layout_args_ok(out, cap, n, src_w, src_h, cw, ch) || speaker < 0 || speaker >= n) return -1;
    const int SH = n == 1 ? 0 : 2 * (ch / 8), m = n - 1;
    for (int k = 0, slot = 0; k < n; k++) {
        int X0 = 0, X1 = cw, Y0 = 0, Y1 = ch - SH;
        if (k != speaker) {
            X0 = 2 * (slot * cw / (2 * m)); X1 = 2 * ((slot + 1) * cw / (2 * m)); Y0 = ch - SH; Y1 = ch;
            slot++;
        }
        if (!fit_centred(out + k, k, src_w, src_h, X0, X1, Y0, Y1, true)) return -1;
    }
    return n;
}
}  // namespace h264mi
