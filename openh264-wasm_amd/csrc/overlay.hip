// overlay.hip -- sprites with an alpha plane blended onto I420 frames on the device (gfx950), as include/h264mi.h
// defines it (h264mi_i420_overlay_dev, h264mi_rgba_to_i420a_dev, h264mi_enc_set_overlays). DESIGN.md §5.6.
//   overlay_kernel       : up to H264MI_OVERLAY_PER_LAUNCH placements per launch -- the standalone call, or an
//                          encoder's overlay list blended into its input area in front of a frame step
//   rgba_to_i420a_kernel : n tight RGBA frames to n tight I420A sprites (Y, Cb, Cr as color.inc's conversion, A = the
//                          fourth byte)
// A placement takes a w x h crop of one sprite 1:1 onto a rectangle of one canvas. Per sample, plain non-negative
// integers:
//     a   = (A * opacity + 128) >> 8                      0..255, A the sprite's alpha there
//     out = (d * (255 - a) + s * a + 127) / 255           d the canvas sample, s the sprite's
// and for a chroma sample a = (a00 + a01 + a10 + a11 + 2) >> 2 over the effective alphas of the four luma positions
// it covers. The division is t = x + 128; (t + (t >> 8)) >> 8, the same value for every x in 0..65025.
// The walk is compose_kernel's with one change: a wave owns a tile of 64 luma columns by H264MI_OVERLAY_ROWS luma rows
// of one placement TOGETHER WITH that tile's chroma (32 columns by 8 rows of Cb and of Cr), so the alpha plane is read
// once and the chroma alpha comes from registers:
//  * the launch's arguments hold the placements (16-bit geometry) and a prefix table of waves per placement; a wave
//    finds its placement by a binary search of that table, all of it scalar.
//  * luma: a lane per column. Two rows at a time: alpha, sprite and canvas of both rows and the chroma rows below them
//    are loaded, then blended, then stored. The two rows' effective alphas are added per lane, then per pair of lanes;
//    chroma lane j takes the sum of lanes 2j and 2j + 1.
//  * chroma: lanes 0..31 are the Cb columns of the tile's chroma row, lanes 32..63 the Cr columns.
//  * a row segment is read as dwords when its first address is a multiple of 4 -- tested per row and per pointer,
//    since with odd pitches (a 19-byte chroma pitch) it changes from row to row -- and then only the groups of four
//    samples that lie inside the segment; everything else as bytes. Stores likewise (compose's rule: only groups wholly
//    inside the rectangle; picture_dev.h's seg_pack and seg_store, apart because a chroma row's pointer differs by lane). Nothing is read outside the crop, nothing is read or written outside the rectangle.
// Order: placements may overlap and the last one is on top. The host cuts the list into launches so that no two
// placements of one launch share a sample of one canvas (overlay_launch_end); launches go to the stream in list
// order, so stream order is z-order and the waves of one launch never touch the same byte. No atomics, no device
// allocation, no copies.
//
// A translation unit and a code object of its own, as quality.hip, scale.hip and compose.hip are. The host runtime (enc_input.inc, capi_enc.inc) reaches it through the functions
// picture_host.h declares.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include "../../include/h264mi.h"
#include "picture_host.h"
#include "picture_dev.h"

namespace h264mi {
#define H264MI_OVERLAY_ROWS 16          // luma rows per wave

struct OverlayItem {  // a placement as the kernel reads it, 24 bytes
    int32_t sprite, canvas;
    uint16_t sx, sy, w, h, dx, dy, opacity, pad;
};
struct OverlayLaunch {
    const uint8_t *spr;
    uint8_t *dst;
    size_t sfb, dfb;                                   // sprite f: spr + f * sfb; canvas c: dst + c * dfb
    int ow, oh, cw, ch;
    int n;
    int first[H264MI_OVERLAY_PER_LAUNCH + 1];          // placement k's waves are first[k] .. first[k + 1] - 1
    OverlayItem item[H264MI_OVERLAY_PER_LAUNCH];
};
static_assert(sizeof(OverlayLaunch) < 2048, "the argument block stays well below 4 KB");

// (x + 127) / 255 for x in 0..65025
PICDEV uint32_t div255(uint32_t x) {
    const uint32_t t = x + 128;
    return (t + (t >> 8)) >> 8;
}
PICDEV uint32_t blend(uint32_t d, uint32_t s, uint32_t a) { return div255(d * (255u - a) + s * a); }

// sample i of the n-sample row segment at p (0 for i >= n): from the aligned dword that holds it when the segment
// starts at a multiple of 4 and the dword lies inside the segment, else a byte
PICDEV uint32_t seg_load(const uint8_t *p, int i, int n) {
    uint32_t v = 0;
    if (i < n) {
        if ((((uintptr_t)p) & 3) == 0 && (i | 3) < n) v = (*(const uint32_t *)(p + (i & ~3)) >> (8 * (i & 3))) & 255u;
        else v = p[i];
    }
    return v;
}
// waves across and down a w x h placement
__host__ __device__ static inline int overlay_nstrip(int w) { return (w + 63) / 64; }
__host__ __device__ static inline int overlay_nseg(int h) { return (h + H264MI_OVERLAY_ROWS - 1) / H264MI_OVERLAY_ROWS; }

__global__ __launch_bounds__(256) void overlay_kernel(OverlayLaunch a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // scalar: what follows from it is per wave
    const int items = a.first[a.n];
    const int cl = lane & 31, cp = lane >> 5;  // the lane's chroma column within the tile, its chroma plane
    const size_t sy_b = (size_t)a.ow * a.oh, sc_b = (size_t)(a.ow >> 1) * (a.oh >> 1);
    const size_t dy_b = (size_t)a.cw * a.ch, dc_b = (size_t)(a.cw >> 1) * (a.ch >> 1);
    const int spc = a.ow >> 1, dpc = a.cw >> 1;  // chroma pitches
    for (int it = (int)blockIdx.x * 4 + wave; it < items; it += (int)gridDim.x * 4) {
        int lo_c = 0, hi_c = a.n;  // first[lo_c] <= it < first[hi_c]
        while (hi_c - lo_c > 1) {
            const int mid_c = (lo_c + hi_c) >> 1;
            if (a.first[mid_c] <= it) lo_c = mid_c; else hi_c = mid_c;
        }
        const OverlayItem c = a.item[lo_c];
        const int k = it - a.first[lo_c];  // the wave's index within the placement
        const int nstrip = overlay_nstrip(c.w);
        const int strip = k % nstrip, seg = k / nstrip;
        const int x0 = strip * 64, y0 = seg * H264MI_OVERLAY_ROWS;       // the tile's origin within the placement, even
        const int n = min(64, (int)c.w - x0), rows = min(H264MI_OVERLAY_ROWS, (int)c.h - y0);  // even, >= 2
        const int nc = n >> 1;
        const uint32_t op = c.opacity;
        const uint8_t *__restrict__ SP = a.spr + (size_t)c.sprite * a.sfb;
        uint8_t *CV = a.dst + (size_t)c.canvas * a.dfb;
        // the tile's first sample in the sprite's luma plane (the alpha plane is sy_b + 2 sc_b further), in the canvas's
        // luma plane, and in this lane's chroma plane of each
        const uint8_t *SY = SP + (size_t)(c.sy + y0) * a.ow + c.sx + x0;
        const uint8_t *SA = SY + sy_b + 2 * sc_b;
        uint8_t *DY = CV + (size_t)(c.dy + y0) * a.cw + c.dx + x0;
        const uint8_t *SC = SP + sy_b + (size_t)cp * sc_b + (size_t)((c.sy + y0) >> 1) * spc + ((c.sx + x0) >> 1);
        uint8_t *DC = CV + dy_b + (size_t)cp * dc_b + (size_t)((c.dy + y0) >> 1) * dpc + ((c.dx + x0) >> 1);
        for (int rp = 0; 2 * rp < rows; rp++) {  // luma rows 2 rp and 2 rp + 1 of the tile, chroma row rp
            const uint8_t *pa0 = SA + (size_t)(2 * rp) * a.ow, *pa1 = pa0 + a.ow;
            const uint8_t *ps0 = SY + (size_t)(2 * rp) * a.ow, *ps1 = ps0 + a.ow;
            uint8_t *pd0 = DY + (size_t)(2 * rp) * a.cw, *pd1 = pd0 + a.cw;
            const uint8_t *psc = SC + (size_t)rp * spc;
            uint8_t *pdc = DC + (size_t)rp * dpc;
            const uint32_t A0 = seg_load(pa0, lane, n), A1 = seg_load(pa1, lane, n);
            const uint32_t s0 = seg_load(ps0, lane, n), s1 = seg_load(ps1, lane, n);
            const uint32_t d0 = seg_load(pd0, lane, n), d1 = seg_load(pd1, lane, n);
            const uint32_t sc = seg_load(psc, cl, nc), dc = seg_load(pdc, cl, nc);
            const uint32_t a0 = (A0 * op + 128u) >> 8, a1 = (A1 * op + 128u) >> 8;  // 0 in lanes beyond the segment
            const uint32_t o0 = blend(d0, s0, a0), o1 = blend(d1, s1, a1);
            const uint32_t v = a0 + a1;
            const uint32_t h = v + __shfl_down(v, 1);             // even lanes: the four alphas of a chroma sample
            const uint32_t ac = (__shfl(h, 2 * cl) + 2u) >> 2;
            const uint32_t oc = blend(dc, sc, ac);
            const uint32_t q0 = seg_pack(o0), q1 = seg_pack(o1), qc = seg_pack(oc);
            seg_store(pd0, lane, n, o0, q0);
            seg_store(pd1, lane, n, o1, q1);
            seg_store(pdc, cl, nc, oc, qc);
        }
    }
}

// One RGBA pixel (R | G << 8 | B << 16 | A << 24) to Y, Cb, Cr: the wrapper's formulas, as color.inc has them
PICDEV uint32_t o_rgb_y(uint32_t p) {
    const int r = p & 255, g = (p >> 8) & 255, b = (p >> 16) & 255;
    return (uint8_t)(((66 * r + 129 * g + 25 * b + 128) >> 8) + 16);
}
PICDEV uint32_t o_rgb_u(uint32_t p) {
    const int r = p & 255, g = (p >> 8) & 255, b = (p >> 16) & 255;
    return (uint8_t)((uint8_t)((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128);
}
PICDEV uint32_t o_rgb_v(uint32_t p) {
    const int r = p & 255, g = (p >> 8) & 255, b = (p >> 16) & 255;
    return (uint8_t)((uint8_t)((112 * r - 94 * g - 18 * b + 128) >> 8) + 128);
}
PICDEV uint32_t o_pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return a | (b << 8) | (c << 16) | (d << 24); }

// n tight RGBA frames (4-byte aligned) -> n tight I420A sprites at any alignment. blockIdx.y strides the frames; a
// thread owns a unit of 4 pixels on 2 rows (2 pixels where w % 4 == 2 ends the row): one 16-byte RGBA access a row
// when the frame is 16-byte aligned, else four of 4 bytes; Y and A as one dword a row and Cb, Cr as two bytes each
// where the unit is whole and the address allows it, bytes otherwise. Chroma from the top-left pixel of each 2x2.
__global__ __launch_bounds__(256) void rgba_to_i420a_kernel(const uint8_t *__restrict__ rgba, uint8_t *__restrict__ out, int w, int h, int n) {
    const int cw = w >> 1, upr = (w + 3) >> 2, units = upr * (h >> 1);
    const size_t yb = (size_t)w * h, cb = (size_t)cw * (h >> 1);
    const size_t fin = yb * 4, fout = 2 * yb + 2 * cb;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint8_t *src = rgba + (size_t)f * fin;
        uint8_t *Y = out + (size_t)f * fout, *U = Y + yb, *V = U + cb, *A = V + cb;
        const bool vec = (((uintptr_t)src) & 15) == 0;
        for (int u = blockIdx.x * 256 + threadIdx.x; u < units; u += gridDim.x * 256) {
            const int by = u / upr, x = (u - by * upr) * 4;
            const int px = min(4, w - x);  // 4 or 2
            const uint32_t *p0 = (const uint32_t *)(src + ((size_t)(2 * by) * w + x) * 4), *p1 = p0 + w;
            uint32_t r0[4], r1[4];
            if (vec && px == 4) {
                const uint4 t0 = *(const uint4 *)p0, t1 = *(const uint4 *)p1;
                r0[0] = t0.x; r0[1] = t0.y; r0[2] = t0.z; r0[3] = t0.w;
                r1[0] = t1.x; r1[1] = t1.y; r1[2] = t1.z; r1[3] = t1.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) { r0[i] = i < px ? p0[i] : 0u; r1[i] = i < px ? p1[i] : 0u; }
            }
            const uint32_t y0 = o_pack4(o_rgb_y(r0[0]), o_rgb_y(r0[1]), o_rgb_y(r0[2]), o_rgb_y(r0[3]));
            const uint32_t y1 = o_pack4(o_rgb_y(r1[0]), o_rgb_y(r1[1]), o_rgb_y(r1[2]), o_rgb_y(r1[3]));
            const uint32_t al0 = o_pack4(r0[0] >> 24, r0[1] >> 24, r0[2] >> 24, r0[3] >> 24);
            const uint32_t al1 = o_pack4(r1[0] >> 24, r1[1] >> 24, r1[2] >> 24, r1[3] >> 24);
            const size_t o = (size_t)(2 * by) * w + x, c = (size_t)by * cw + (x >> 1);
            uint8_t *dst4[4] = {Y + o, Y + o + w, A + o, A + o + w};
            const uint32_t val4[4] = {y0, y1, al0, al1};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (px == 4 && (((uintptr_t)dst4[i]) & 3) == 0) *(uint32_t *)dst4[i] = val4[i];
                else for (int b = 0; b < px; b++) dst4[i][b] = (uint8_t)(val4[i] >> (8 * b));
            }
            U[c] = (uint8_t)o_rgb_u(r0[0]); V[c] = (uint8_t)o_rgb_v(r0[0]);
            if (px == 4) { U[c + 1] = (uint8_t)o_rgb_u(r0[2]); V[c + 1] = (uint8_t)o_rgb_v(r0[2]); }
        }
    }
}

// arguments of a conversion to sprites
bool rgba_to_i420a_args_ok(int w, int h, int n) { return canvas_ok(w, h) && n > 0; }
int launch_rgba_to_i420a(const uint8_t *d_rgba, int w, int h, int n, uint8_t *d_out, hipStream_t s) {
    const int ny = std::min(n, 256);
    const long long units = (long long)((w + 3) / 4) * (h / 2);
    const long long bx = std::max(1LL, std::min((units + 255) / 256, (long long)(PIC_MAX_BLOCKS / ny)));
    (void)hipGetLastError();
    hipLaunchKernelGGL(rgba_to_i420a_kernel, dim3((unsigned)bx, (unsigned)ny), dim3(256), 0, s, d_rgba, d_out, w, h, n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// arguments of an overlay call, everything but the pointers' values: counts, sizes and every placement's fields
bool overlay_args_ok(int cw, int ch, int ncanvas, int ow, int oh, int nsprites, const h264mi_overlay *ov, int nov) {
    if (!ov || ncanvas <= 0 || nsprites <= 0 || nov <= 0 || nov > PIC_MAX_LIST) return false;
    if (!canvas_ok(cw, ch) || !canvas_ok(ow, oh)) return false;
    for (int k = 0; k < nov; k++) {
        const h264mi_overlay &p = ov[k];
        if (p.sprite < 0 || p.sprite >= nsprites || p.canvas < 0 || p.canvas >= ncanvas) return false;
        if ((p.sx | p.sy | p.w | p.h | p.dx | p.dy) & 1) return false;
        if (p.w < 2 || p.h < 2 || p.sx < 0 || p.sy < 0 || p.dx < 0 || p.dy < 0) return false;
        if (p.sx > ow || p.sy > oh || p.w > ow - p.sx || p.h > oh - p.sy) return false;  // sx <= ow first: no overflow
        if (p.dx > cw || p.dy > ch || p.w > cw - p.dx || p.h > ch - p.dy) return false;
        if (p.opacity < 0 || p.opacity > 256 || p.reserved != 0) return false;
    }
    return true;
}
// the launch that starts at placement k0 ends before the value returned: the first placement that shares a sample of
// a canvas with one already in the launch, or H264MI_OVERLAY_PER_LAUNCH placements, or the list's end
int overlay_launch_end(const h264mi_overlay *ov, int nov, int k0) {
    int k1 = k0 + 1;
    for (; k1 < nov && k1 - k0 < H264MI_OVERLAY_PER_LAUNCH; k1++) {
        const h264mi_overlay &p = ov[k1];
        bool shared = false;
        for (int j = k0; j < k1 && !shared; j++) {
            const h264mi_overlay &q = ov[j];
            shared = p.canvas == q.canvas && rects_share(p.dx, p.dy, p.w, p.h, q.dx, q.dy, q.w, q.h);
        }
        if (shared) break;
    }
    return k1;
}
// placements (as overlay_args_ok accepts them) onto the canvases at dst, launch after launch in list order. The table
// is filled here and not by picture_host.h's fill_cell_table: a placement is another structure than a cell (one size,
// an opacity) and its launches end where overlay_launch_end says, not after a fixed count
int launch_overlay_i420(uint8_t *dst, int cw, int ch, const uint8_t *spr, int ow, int oh, const h264mi_overlay *ov, int nov, hipStream_t s) {
    OverlayLaunch a{};
    a.spr = spr; a.dst = dst; a.sfb = i420a_bytes(ow, oh); a.dfb = i420_bytes(cw, ch);
    a.ow = ow; a.oh = oh; a.cw = cw; a.ch = ch;
    (void)hipGetLastError();
    for (int k0 = 0; k0 < nov;) {
        const int k1 = overlay_launch_end(ov, nov, k0);
        a.n = k1 - k0;
        a.first[0] = 0;
        for (int k = 0; k < a.n; k++) {
            const h264mi_overlay &p = ov[k0 + k];
            a.item[k] = OverlayItem{p.sprite, p.canvas, (uint16_t)p.sx, (uint16_t)p.sy, (uint16_t)p.w, (uint16_t)p.h,
                                    (uint16_t)p.dx, (uint16_t)p.dy, (uint16_t)p.opacity, 0};
            a.first[k + 1] = a.first[k] + overlay_nstrip(p.w) * overlay_nseg(p.h);  // at most 128 * 512 a placement, 64 of them
        }
        hipLaunchKernelGGL(overlay_kernel, dim3(launch_blocks(a.first[a.n])), dim3(256), 0, s, a);
        k0 = k1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace h264mi
