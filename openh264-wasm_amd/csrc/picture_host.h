// picture_host.h -- the host half that the picture code objects (scale.hip, compose.hip, overlay.hip, upscale.hip, orient.hip,
// pixfmt.hip, pixdeep.hip, colorspace.hip, denoise.hip, scenecut.hip, deinterlace.hip, spatial.hip, levels.hip, warp.hip) and the runtime (runtime_enc.inc, enc_input.inc, runtime_dec.inc, capi_enc.inc, capi_dec.inc) share: byte counts, the limits of a call, the checks of a cell
// list, the cell table of a launch, the layouts' fit, and the declaration of every function a code object exports to
// the runtime. Host only: nothing here is compiled for the device but the plain 24-byte PictureCell, which the compose
// and upscale launch structs hold, and the plain 60-byte CsCoef, which the colour launches hold. DESIGN.md §5.8.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stddef.h>
#include <stdint.h>
#include "../../include/h264mi.h"

struct EncDesc;  // h264mi_types.h
struct EncState;
struct DecDesc;
struct DecInput;

namespace h264mi {

// ---- limits of a picture call
// source side. Area average (scale, compose): the numerator 255 * 4096^2 + 4096^2 / 2 stays below 2^32. Enlarging:
// the phase numerator 16 N + 33 q stays below 2^31 with q <= PIC_MAX_SIDE
constexpr int PIC_MAX_SRC = 4096;
// canvas, destination and sprite side: a geometry field of a device cell or placement fits 16 bits
constexpr int PIC_MAX_SIDE = 8192;
// cells or placements per call; H264MI_COMPOSE_CELLS, H264MI_UPSCALE_PER_LAUNCH or H264MI_OVERLAY_PER_LAUNCH of them
// travel in one launch's arguments
constexpr int PIC_MAX_LIST = 4096;
// blocks per launch: 8 blocks of 256 on each of 256 CUs; the rest is a stride loop
constexpr int PIC_MAX_BLOCKS = 2048;

// ---- bytes
static inline size_t i420_bytes(int w, int h) { return (size_t)w * h + 2 * (size_t)(w / 2) * (h / 2); }
static inline size_t i420a_bytes(int w, int h) { return 2 * (size_t)w * h + 2 * (size_t)(w / 2) * (h / 2); }
// whether abytes bytes at a and bbytes bytes at b share a byte
static inline bool byte_ranges_overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bbytes && b0 < a0 + abytes;
}
// the same for na tight aw x ah I420 frames at a and nb tight bw x bh ones at b
static inline bool i420_ranges_overlap(const void *a, int aw, int ah, int na, const void *b, int bw, int bh, int nb) {
    return byte_ranges_overlap(a, (size_t)na * i420_bytes(aw, ah), b, (size_t)nb * i420_bytes(bw, bh));
}

// ---- geometry
static inline bool side_ok(int v, int max) { return v >= 2 && v <= max && !(v & 1); }
// a canvas, destination or sprite: even sides from 2 within PIC_MAX_SIDE
static inline bool canvas_ok(int w, int h) { return side_ok(w, PIC_MAX_SIDE) && side_ok(h, PIC_MAX_SIDE); }
// a call that takes src_w x src_h pictures to cw x ch ones: the same, and the source within PIC_MAX_SRC
static inline bool sides_ok(int cw, int ch, int src_w, int src_h) {
    return canvas_ok(cw, ch) && side_ok(src_w, PIC_MAX_SRC) && side_ok(src_h, PIC_MAX_SRC);
}
static inline bool filter_ok(int filter) { return filter == H264MI_FILTER_BILINEAR || filter == H264MI_FILTER_BICUBIC; }
// whether two rectangles share a sample (touching ones do not)
static inline bool rects_share(int ax, int ay, int aw, int ah, int bx, int by, int bw, int bh) {
    return ax < bx + bw && bx < ax + aw && ay < by + bh && by < ay + ah;
}
// blocks of four waves for a launch's waves
static inline unsigned launch_blocks(long long waves) { return (unsigned)std::min((waves + 3) / 4, (long long)PIC_MAX_BLOCKS); }

// ---- pixel formats and pitched layouts (include/h264mi.h)
constexpr int PIX_MAX_PITCH = 65536;
// planes of a format, 0 for an unknown one (ids 5..15 are unassigned)
static inline int pix_planes(int pix) {
    switch (pix) {
    case H264MI_PIX_I420: case H264MI_PIX_I422: case H264MI_PIX_I444: case H264MI_PIX_I010: case H264MI_PIX_I210: return 3;
    case H264MI_PIX_NV12: case H264MI_PIX_NV21: case H264MI_PIX_NV16: case H264MI_PIX_P010: case H264MI_PIX_P210: return 2;
    case H264MI_PIX_YUY2: case H264MI_PIX_UYVY: case H264MI_PIX_Y800: case H264MI_PIX_V210: return 1;
    default: return 0;
    }
}
// the unit of a format: every used pitch and offset, frame_stride and the layout side's base are multiples of it. -1 for
// an unknown format
static inline int pix_unit(int pix) {
    if (pix_planes(pix) == 0) return -1;
    return pix == H264MI_PIX_V210 ? 4 : pix >= H264MI_PIX_P010 ? 2 : 1;
}
// the formats of pixdeep.hip (ids 16..24); the others are pixfmt.hip's
static inline bool pix_is_deep(int pix) { return pix >= H264MI_PIX_I422; }
// row bytes and rows of plane p < pix_planes(pix) of a w x h frame
static inline void pix_plane_size(int pix, int p, int w, int h, int *row_bytes, int *rows) {
    *rows = h;
    switch (pix) {
    case H264MI_PIX_YUY2: case H264MI_PIX_UYVY: *row_bytes = 2 * w; return;
    case H264MI_PIX_V210: *row_bytes = 16 * ((w + 5) / 6); return;
    case H264MI_PIX_I444: case H264MI_PIX_Y800: case H264MI_PIX_NV16: *row_bytes = w; return;
    case H264MI_PIX_I422: *row_bytes = p == 0 ? w : w / 2; return;
    case H264MI_PIX_P210: *row_bytes = 2 * w; return;
    case H264MI_PIX_I210: *row_bytes = p == 0 ? 2 * w : w; return;
    case H264MI_PIX_P010: *row_bytes = 2 * w; break;
    case H264MI_PIX_I010: *row_bytes = p == 0 ? 2 * w : w; break;
    case H264MI_PIX_I420: *row_bytes = p == 0 ? w : w / 2; break;
    default: *row_bytes = w; break;  // NV12, NV21
    }
    if (p > 0) *rows = h / 2;  // the 4:2:0 formats
}
// the span of a layout for w x h frames -- every rule of h264mi_pix_layout_ok but the two frame_stride ones -- or -1. 64-bit
// arithmetic that cannot overflow: a plane's extent is at most 8191 * 65536 + 21856 < 2^30, and an offset that would
// carry its end past INT64_MAX is refused before the sum is formed
static inline int64_t pix_span(const h264mi_pix_layout *L, int w, int h) {
    if (!L || !canvas_ok(w, h)) return -1;
    const int np = pix_planes(L->pix);
    if (np == 0) return -1;
    const int um = pix_unit(L->pix) - 1;
    int64_t end[3] = {0, 0, 0}, span = 0;
    for (int p = 0; p < 3; p++) {
        if (p >= np) {
            if (L->pitch[p] != 0 || L->offset[p] != 0) return -1;
            continue;
        }
        int rb, rows;
        pix_plane_size(L->pix, p, w, h, &rb, &rows);
        if (L->pitch[p] < rb || L->pitch[p] > PIX_MAX_PITCH || L->offset[p] < 0) return -1;
        if ((L->pitch[p] & um) || (L->offset[p] & um)) return -1;
        const int64_t extent = (int64_t)(rows - 1) * L->pitch[p] + rb;
        if (L->offset[p] > INT64_MAX - extent) return -1;
        end[p] = L->offset[p] + extent;
        span = std::max(span, end[p]);
    }
    for (int p = 1; p < np; p++)
        for (int q = 0; q < p; q++)
            if (L->offset[p] < end[q] && L->offset[q] < end[p]) return -1;
    return span;
}
static inline bool pix_layout_ok(const h264mi_pix_layout *L, int w, int h) {
    const int64_t span = pix_span(L, w, h);
    return span >= 0 && L->frame_stride >= span && !(L->frame_stride & (pix_unit(L->pix) - 1));
}
static inline int pix_layout_tight(h264mi_pix_layout *out, int pix, int w, int h) {
    const int np = pix_planes(pix);
    if (!out || np == 0 || !canvas_ok(w, h)) return -1;
    h264mi_pix_layout L{};
    L.pix = pix;
    int64_t at = 0;
    for (int p = 0; p < np; p++) {
        int rb, rows;
        pix_plane_size(pix, p, w, h, &rb, &rows);
        if (pix == H264MI_PIX_V210) rb = 128 * ((w + 47) / 48);  // the format's customary row alignment
        L.pitch[p] = rb;
        L.offset[p] = at;
        at += (int64_t)rb * rows;
    }
    L.frame_stride = at;
    *out = L;
    return 0;
}
// whether n frames of a good layout at a and n tight w x h I420 frames at b share a byte; a layout side too long for
// any address space (n * frame_stride beyond 2^63) counts as overlapping
static inline bool pix_ranges_overlap(const void *a, const h264mi_pix_layout &L, const void *b, int w, int h, int n) {
    const unsigned __int128 abytes = (unsigned __int128)(uint64_t)L.frame_stride * (unsigned)n;
    if (abytes >> 63) return true;
    const unsigned __int128 a0 = (uintptr_t)a, b0 = (uintptr_t)b, bbytes = (unsigned __int128)i420_bytes(w, h) * (unsigned)n;
    return a0 < b0 + bbytes && b0 < a0 + abytes;
}
// arguments of a conversion call, everything but the pointers' values
static inline bool pix_args_ok(const h264mi_pix_layout *L, int w, int h, int n) { return n > 0 && pix_layout_ok(L, w, h); }
// the layout side's base pointer of a good layout: a multiple of the format's unit
static inline bool pix_base_ok(const void *base, const h264mi_pix_layout &L) { return !((uintptr_t)base & (uintptr_t)(pix_unit(L.pix) - 1)); }
static inline bool pixopt_ok(const h264mi_pixopt *o) {
    return o && (uint32_t)o->depth <= 2 && !(o->reserved[0] | o->reserved[1] | o->reserved[2]);
}

// ---- colour specifications (include/h264mi.h)
// one row of the header's table, as the kernels of colorspace.hip take it in their arguments
struct CsCoef {
    int32_t fy[3], fu[3], fv[3];  // RGB -> Y, Cb, Cr, 8 fractional bits
    int32_t yo;                   // luma offset
    int32_t iy, rv, gu, gv, bu;   // Y, Cb, Cr -> RGB, 8 fractional bits
};
static_assert(sizeof(CsCoef) == 60, "the launch structs count on it");
static inline bool colorspec_ok(const h264mi_colorspec *s) {
    return s && !((uint32_t)s->matrix > 1 || (uint32_t)s->range > 1 || (uint32_t)s->chroma_down > 1 || (uint32_t)s->chroma_up > 1);
}
static inline bool colorspec_default(const h264mi_colorspec &s) { return (s.matrix | s.range | s.chroma_down | s.chroma_up) == 0; }
// the table: index matrix * 2 + range of a good specification. Every FU and FV row sums to 0, FY to 220 (limited) or 256 (full)
static inline const CsCoef &cs_coef(int matrix, int range) {
    static const CsCoef T[4] = {
        {{66, 129, 25}, {-38, -74, 112}, {112, -94, -18}, 16, 298, 409, 100, 208, 516},   // 601 limited: the wrapper's
        {{77, 150, 29}, {-43, -85, 128}, {128, -107, -21}, 0, 256, 359, 88, 183, 454},    // 601 full
        {{47, 157, 16}, {-26, -86, 112}, {112, -102, -10}, 16, 298, 459, 55, 136, 541},   // 709 limited
        {{54, 183, 19}, {-29, -99, 128}, {128, -116, -12}, 0, 256, 403, 48, 120, 475},    // 709 full
    };
    return T[(matrix & 1) * 2 + (range & 1)];
}
// arguments of a conversion call under a specification, everything but the pointers' values
static inline bool cs_args_ok(int w, int h, int n, const h264mi_colorspec *s) { return n > 0 && canvas_ok(w, h) && colorspec_ok(s); }

// ---- the temporal denoiser (include/h264mi.h)
constexpr int DENOISE_MAX_STRENGTH = 224, DENOISE_MAX_REACH = 32, DENOISE_MAX_MOTION = 1020;
static inline bool denoise_ok(const h264mi_denoise *p) {
    return p && p->strength_y >= 0 && p->strength_y <= DENOISE_MAX_STRENGTH && p->strength_c >= 0 && p->strength_c <= DENOISE_MAX_STRENGTH &&
           p->reach >= 1 && p->reach <= DENOISE_MAX_REACH && p->motion >= 0 && p->motion <= DENOISE_MAX_MOTION;
}
// k of the sample rule for a difference a of good parameters: K (T - a) / T below the reach, 0 from it on
static inline int denoise_k(int K, int T, int a) { return a < T ? K * (T - a) / T : 0; }
// the tables of a launch: byte a of k[0..7] is luma's k[a], of k[8..15] chroma's, a = 0..31 (every a >= 32 has k = 0)
struct DenoiseTables { uint32_t k[16]; };
static_assert(sizeof(DenoiseTables) == 64, "the launch struct counts on it");
static inline void denoise_tables(DenoiseTables *t, const h264mi_denoise &p) {
    for (int pl = 0; pl < 2; pl++)
        for (int w = 0; w < 8; w++) {
            uint32_t v = 0;
            for (int j = 0; j < 4; j++) v |= (uint32_t)denoise_k(pl ? p.strength_c : p.strength_y, p.reach, 4 * w + j) << (8 * j);
            t->k[8 * pl + w] = v;
        }
}
// arguments of a denoise call, the pointers' values included: good parameters, even sides from 2 within PIC_MAX_SIDE,
// n >= 1, statistics at a multiple of 4; each destination exactly cur, exactly prev, or disjoint from both sources, the
// statistics and the other destination; the sources equal or disjoint; the statistics disjoint from the sources
static inline bool denoise_args_ok(const void *dst, const void *dst2, const void *cur, const void *prev, int w, int h, int n,
                                   const h264mi_denoise *p, const void *stats) {
    if (!dst || !cur || !prev || n < 1 || !canvas_ok(w, h) || !denoise_ok(p) || ((uintptr_t)stats & 3)) return false;
    const size_t nb = (size_t)n * i420_bytes(w, h), sb = 16 * (size_t)n;
    if (cur != prev && byte_ranges_overlap(cur, nb, prev, nb)) return false;
    const void *d[2] = {dst, dst2};
    for (int k = 0; k < 2; k++) {
        if (!d[k]) continue;
        if (d[k] != cur && byte_ranges_overlap(d[k], nb, cur, nb)) return false;
        if (d[k] != prev && byte_ranges_overlap(d[k], nb, prev, nb)) return false;
        if (stats && byte_ranges_overlap(d[k], nb, stats, sb)) return false;
    }
    if (dst2 && byte_ranges_overlap(dst, nb, dst2, nb)) return false;  // equal ones too
    if (stats && (byte_ranges_overlap(cur, nb, stats, sb) || byte_ranges_overlap(prev, nb, stats, sb))) return false;
    return true;
}

// ---- the scene-cut detector (include/h264mi.h)
constexpr int SCENECUT_MAX_LEVEL = 1020, SCENECUT_MAX_SHARE = 256, SCENECUT_MAX_GAP = 65535;
static inline bool scenecut_ok(const h264mi_scenecut *p) {
    return p && p->level >= 0 && p->level <= SCENECUT_MAX_LEVEL && p->share >= 0 && p->share <= SCENECUT_MAX_SHARE && p->min_gap >= 0 &&
           p->min_gap <= SCENECUT_MAX_GAP && p->max_gap >= 0 && p->max_gap <= SCENECUT_MAX_GAP && (uint32_t)p->compensate <= 1;
}
static inline int thumb_side(int v) { return (v + 3) / 4; }
static inline size_t thumb_bytes(int w, int h) { return (size_t)thumb_side(w) * thumb_side(h); }
// the cut test of a frame's statistics, the one expression of the host and of the decision kernel: changed <= 65536
// blocks and share <= 256, so neither product leaves 32 bits
__host__ __device__ static inline bool scenecut_is_cut(int share, uint32_t changed, uint32_t blocks) {
    return share > 0 && 256u * changed > (uint32_t)share * blocks;
}
// arguments of a scene-cut call, the pointers' values included: good parameters, even sides from 2 within
// PIC_MAX_SIDE, n >= 1, an output, statistics only with previous thumbnails and at a multiple of 4; of the frames, the
// two thumbnail ranges and the statistics no two share a byte, but that thumb_out may be exactly thumb_prev
static inline bool scenecut_args_ok(const void *stats, const void *thumb_out, const void *cur, const void *thumb_prev, int w, int h, int n,
                                    const h264mi_scenecut *p) {
    if (!cur || (!stats && !thumb_out) || (stats && !thumb_prev) || n < 1 || !canvas_ok(w, h) || !scenecut_ok(p) || ((uintptr_t)stats & 3))
        return false;
    const size_t fb = (size_t)n * i420_bytes(w, h), tb = (size_t)n * thumb_bytes(w, h), sb = 32 * (size_t)n;
    const void *r[4] = {cur, thumb_out, thumb_prev, stats};
    const size_t rb[4] = {fb, tb, tb, sb};
    for (int a = 0; a < 4; a++)
        for (int b = a + 1; b < 4; b++) {
            if (!r[a] || !r[b]) continue;
            if (a == 1 && b == 2 && r[a] == r[b]) continue;
            if (byte_ranges_overlap(r[a], rb[a], r[b], rb[b])) return false;
        }
    return true;
}

// ---- the deinterlacer (include/h264mi.h)
constexpr int DEINTERLACE_MAX_COMB = 255;
static inline bool deinterlace_ok(const h264mi_deinterlace *p) {
    return p && (uint32_t)p->parity <= 1 && (uint32_t)p->spatial <= 1 && (uint32_t)p->temporal <= 1 && p->comb_level >= 0 &&
           p->comb_level <= DEINTERLACE_MAX_COMB;
}
// arguments of a deinterlace call, the pointers' values included: good parameters, the geometry limits of the denoiser,
// n >= 1, statistics at a multiple of 4. Of the written ranges (dst, prev_out, the statistics) each is disjoint from
// every other range, but that dst may be exactly cur and prev_out exactly prev; the two read ranges may overlap in
// any way
static inline bool deinterlace_args_ok(const void *dst, const void *prev_out, const void *cur, const void *prev, int w, int h, int n,
                                       const h264mi_deinterlace *p, const void *stats) {
    if (!dst || !cur || n < 1 || !canvas_ok(w, h) || !deinterlace_ok(p) || ((uintptr_t)stats & 3)) return false;
    const size_t nb = (size_t)n * i420_bytes(w, h), sb = 16 * (size_t)n;
    const void *r[5] = {dst, prev_out, stats, cur, prev};  // the first three are written
    const size_t rb[5] = {nb, nb, sb, nb, nb};
    for (int a = 0; a < 3; a++)
        for (int b = a + 1; b < 5; b++) {
            if (!r[a] || !r[b]) continue;
            if (((a == 0 && b == 3) || (a == 1 && b == 4)) && r[a] == r[b]) continue;
            if (byte_ranges_overlap(r[a], rb[a], r[b], rb[b])) return false;
        }
    return true;
}

// ---- the spatial filter and the privacy masks (include/h264mi.h)
constexpr int SPATIAL_MAX_RADIUS = 3, SPATIAL_MIN_AMOUNT = -64, SPATIAL_MAX_AMOUNT = 255, SPATIAL_MAX_CORE = 255;
static inline bool spatial_ok(const h264mi_spatial *p) {
    return p && p->radius_y >= 0 && p->radius_y <= SPATIAL_MAX_RADIUS && p->radius_c >= 0 && p->radius_c <= SPATIAL_MAX_RADIUS &&
           p->amount_y >= SPATIAL_MIN_AMOUNT && p->amount_y <= SPATIAL_MAX_AMOUNT && p->amount_c >= SPATIAL_MIN_AMOUNT &&
           p->amount_c <= SPATIAL_MAX_AMOUNT && p->core >= 0 && p->core <= SPATIAL_MAX_CORE;
}
// a good setting that changes no sample: each plane kind has r == 0 or amount == 0
static inline bool spatial_inert(const h264mi_spatial &p) {
    return (p.radius_y == 0 || p.amount_y == 0) && (p.radius_c == 0 || p.amount_c == 0);
}
// row weight k = 0..2r of the binomial of radius r = 1..3; the weights of a row sum to 4^r
__host__ __device__ static inline int spatial_weight(int r, int k) {
    return r == 1 ? (k == 1 ? 2 : 1) : r == 2 ? (k == 2 ? 6 : (k & 1) ? 4 : 1) : (k == 3 ? 20 : (k == 2 || k == 4) ? 15 : (k == 1 || k == 5) ? 6 : 1);
}
// the sample rule: c the source sample, l the low-pass there
__host__ __device__ static inline int spatial_sample(int c, int l, int amount, int core) {
    const int d = c - l;
    if (amount > 0 && (d < 0 ? -d : d) <= core) return c;
    const int o = c + ((amount * d + 32) >> 6);
    return o < 0 ? 0 : o > 255 ? 255 : o;
}
// arguments of a spatial call, the pointers' values included
static inline bool spatial_args_ok(const void *dst, const void *src, int w, int h, int n, const h264mi_spatial *p) {
    if (!dst || !src || n < 1 || !canvas_ok(w, h) || !spatial_ok(p)) return false;
    const size_t nb = (size_t)n * i420_bytes(w, h);
    return !byte_ranges_overlap(dst, nb, src, nb);
}
// a list of privacy masks for nframes frames of w x h, everything but the frames' pointer. No entry is read before list
// and n are known to be good
static inline bool privacy_ok(const h264mi_privacy *list, int n, int w, int h, int nframes) {
    if (!list || n <= 0 || n > PIC_MAX_LIST || nframes < 1 || !canvas_ok(w, h)) return false;
    for (int k = 0; k < n; k++) {
        const h264mi_privacy &m = list[k];
        if (m.frame < 0 || m.frame >= nframes || ((m.x | m.y | m.w | m.h) & 1)) return false;
        if (m.x < 0 || m.y < 0 || m.x > w || m.y > h || m.w < 2 || m.h < 2 || m.w > w - m.x || m.h > h - m.y) return false;
        if (m.mode == H264MI_PRIVACY_PIXELATE) {
            if (m.block != 4 && m.block != 8 && m.block != 16 && m.block != 32 && m.block != 64) return false;
        } else if (m.mode == H264MI_PRIVACY_FILL) {
            if ((uint32_t)m.fill_y > 255 || (uint32_t)m.fill_cb > 255 || (uint32_t)m.fill_cr > 255) return false;
        } else {
            return false;
        }
    }
    for (int k = 1; k < n; k++)
        for (int j = 0; j < k; j++)
            if (list[k].frame == list[j].frame && rects_share(list[k].x, list[k].y, list[k].w, list[k].h, list[j].x, list[j].y, list[j].w, list[j].h))
                return false;
    return true;
}

// ---- histograms, level tables and automatic levels (include/h264mi.h)
constexpr int LEVELS_MAX_CLIP = 4096, LEVELS_MIN_GAIN = 64, LEVELS_MAX_GAIN = 1024, LEVELS_MAX_SPEED = 256;
constexpr size_t LEVELS_HIST_BYTES = 768 * sizeof(uint32_t), LEVELS_LUT_BYTES = 768;
static inline bool levels_ok(const h264mi_levels *p) {
    if (!p || (p->mode != H264MI_LEVELS_AUTO && p->mode != H264MI_LEVELS_FIXED)) return false;
    if (p->clip_lo < 0 || p->clip_lo > LEVELS_MAX_CLIP || p->clip_hi < 0 || p->clip_hi > LEVELS_MAX_CLIP) return false;
    if ((uint32_t)p->in_lo > 255 || (uint32_t)p->in_hi > 255 || (uint32_t)p->out_lo > 255 || (uint32_t)p->out_hi > 255) return false;
    if (p->out_lo >= p->out_hi || (p->mode == H264MI_LEVELS_FIXED && p->in_lo >= p->in_hi)) return false;
    return p->max_gain >= LEVELS_MIN_GAIN && p->max_gain <= LEVELS_MAX_GAIN && p->speed >= 1 && p->speed <= LEVELS_MAX_SPEED &&
           (uint32_t)p->sat <= 255;
}
// a good setting whose tables are the identity between the ends and on chroma: "off" for an encoder
static inline bool levels_inert(const h264mi_levels &p) {
    return p.mode == H264MI_LEVELS_FIXED && p.in_lo == p.out_lo && p.in_hi == p.out_hi && p.sat == 64;
}
// the thresholds of the measured ends: the only 64-bit arithmetic of the rule
static inline uint32_t levels_clip_count(int clip, int w, int h) { return (uint32_t)(((uint64_t)clip * ((uint64_t)w * h)) >> 16); }
// a smoothed end after a frame whose measured end is m
__host__ __device__ static inline int levels_follow(int s, int m, int speed) { return s + ((((m << 8) - s) * speed) >> 8); }
// the effective ends of AUTO from the smoothed ones
__host__ __device__ static inline void levels_limit(int lo_s, int hi_s, int R, int max_gain, int &lo_e, int &hi_e) {
    int min_span = (R * 64 * 256) / max_gain;
    if (min_span < 16) min_span = 16;
    if (hi_s - lo_s < min_span) { lo_e = (lo_s + hi_s - min_span) >> 1; hi_e = lo_e + min_span; }
    else { lo_e = lo_s; hi_e = hi_s; }
}
// the table entries of value v
__host__ __device__ static inline int levels_luma(int v, int lo_e, int hi_e, int out_lo, int out_hi) {
    const int t = (v << 8) - lo_e, span = hi_e - lo_e, R = out_hi - out_lo;
    if (t <= 0) return out_lo;
    const int o = out_lo + (t * R + span / 2) / span;
    return o < out_hi ? o : out_hi;
}
__host__ __device__ static inline int levels_chroma(int v, int sat) {
    const int o = 128 + (((v - 128) * sat + 32) >> 6);
    return o < 0 ? 0 : o > 255 ? 255 : o;
}
// arguments of the three calls, the pointers' values included. dst == src, or no byte in common
static inline bool hist_args_ok(const void *hist, const void *frames, int w, int h, int n) {
    if (!hist || !frames || n < 1 || !canvas_ok(w, h) || ((uintptr_t)hist & 3)) return false;
    return !byte_ranges_overlap(hist, (size_t)n * LEVELS_HIST_BYTES, frames, (size_t)n * i420_bytes(w, h));
}
static inline bool lut_args_ok(const void *dst, const void *src, int w, int h, int n, const void *luts, int per_frame) {
    if (!dst || !src || !luts || n < 1 || !canvas_ok(w, h) || (per_frame != 0 && per_frame != 1)) return false;
    const size_t nb = (size_t)n * i420_bytes(w, h);
    if (dst != src && byte_ranges_overlap(dst, nb, src, nb)) return false;
    return !byte_ranges_overlap(dst, nb, luts, (per_frame ? (size_t)n : 1) * LEVELS_LUT_BYTES);
}
static inline size_t levels_work_bytes(int n) { return (size_t)n * (LEVELS_HIST_BYTES + LEVELS_LUT_BYTES); }
static inline bool levels_args_ok(const void *dst, const void *src, int w, int h, int n, const h264mi_levels *p, const void *state,
                                  const void *record, const void *work) {
    if (!dst || !src || !work || n < 1 || !canvas_ok(w, h) || !levels_ok(p)) return false;
    if ((((uintptr_t)state) | ((uintptr_t)record) | ((uintptr_t)work)) & 3) return false;
    const size_t nb = (size_t)n * i420_bytes(w, h);
    if (dst != src && byte_ranges_overlap(dst, nb, src, nb)) return false;
    const void *r[5] = {dst, src, work, state, record};
    const size_t rb[5] = {nb, nb, levels_work_bytes(n), 16 * (size_t)n, 32 * (size_t)n};
    for (int a = 0; a < 5; a++)
        for (int b = (a == 0 ? 2 : a + 1); b < 5; b++) {  // dst against src is settled above
            if (!r[a] || !r[b]) continue;
            if (byte_ranges_overlap(r[a], rb[a], r[b], rb[b])) return false;
        }
    return true;
}

// ---- the sixteen-phase interpolation weights (upscale.hip, warp.hip; include/h264mi.h)
// the four weights of phase f (0..15), sum 8192
__host__ __device__ static inline void up_weights(int f, bool cubic, int *w) {
    if (cubic) {
        const int f2 = f * f, f3 = f2 * f;
        w[0] = -f3 + 32 * f2 - 256 * f;
        w[1] = 3 * f3 - 80 * f2 + 8192;
        w[2] = -3 * f3 + 64 * f2 + 256 * f;
        w[3] = f3 - 16 * f2;
    } else {
        w[0] = 0; w[1] = (16 - f) * 512; w[2] = f * 512; w[3] = 0;
    }
}

// ---- the mesh warp (include/h264mi.h)
constexpr int WARP_MIN_GRID = 3, WARP_MAX_GRID = 5;
constexpr int WARP_POINT_MAX = 1 << 18;  // a control point's coordinates are clamped to +-this, in sixteenths of a sample
// the radial builder's limits: with them every product of its rule stays inside 64 bits (warp.hip has the sums)
constexpr int WARP_RADIAL_MAX_CENTRE = 1 << 18, WARP_RADIAL_MAX_K = 1 << 20;
constexpr int64_t WARP_RADIAL_MAX_R2 = (int64_t)1 << 40, WARP_RADIAL_MAX_Q = (int64_t)1 << 24;
static inline bool warp_grid_ok(int grid_log2) { return grid_log2 >= WARP_MIN_GRID && grid_log2 <= WARP_MAX_GRID; }
static inline bool warp_ok(const h264mi_warp *p) {
    return p && filter_ok(p->filter) && (p->edge == H264MI_WARP_CLAMP || p->edge == H264MI_WARP_FILL) && (uint32_t)p->fill_y <= 255 &&
           (uint32_t)p->fill_u <= 255 && (uint32_t)p->fill_v <= 255 && warp_grid_ok(p->grid_log2);
}
// control points across or down a destination side
static inline int warp_mesh_side(int d, int grid_log2) { return ((d + (1 << grid_log2) - 1) >> grid_log2) + 1; }
static inline size_t warp_mesh_bytes(int dw, int dh, int grid_log2) {
    return (size_t)warp_mesh_side(dw, grid_log2) * warp_mesh_side(dh, grid_log2) * 2 * sizeof(int32_t);
}
// arguments of a warp call, the pointers' values included. Both pictures are canvases (sides_ok would hold the source
// to PIC_MAX_SRC, the limit of the resamplers whose arithmetic grows with the source side; the warp's does not)
static inline bool warp_args_ok(const void *dst, int dw, int dh, const void *src, int sw, int sh, int n, const void *mesh, int mesh_per_frame,
                                const h264mi_warp *p) {
    if (!dst || !src || !mesh || n < 1 || !canvas_ok(dw, dh) || !canvas_ok(sw, sh) || !warp_ok(p)) return false;
    if (((uintptr_t)mesh & 3) || (mesh_per_frame != 0 && mesh_per_frame != 1)) return false;
    const size_t db = (size_t)n * i420_bytes(dw, dh);
    return !byte_ranges_overlap(dst, db, src, (size_t)n * i420_bytes(sw, sh)) &&
           !byte_ranges_overlap(dst, db, mesh, (mesh_per_frame ? (size_t)n : 1) * warp_mesh_bytes(dw, dh, p->grid_log2));
}

// ---- cell lists
// the kind of a cell: 0 shrinking (equal sizes included), 1 enlarging, -1 one axis each way
static inline int cell_kind(const h264mi_cell &c) {
    if (c.dw <= c.sw && c.dh <= c.sh) return 0;
    if (c.dw >= c.sw && c.dh >= c.sh) return 1;
    return -1;
}
// arguments of a call that takes a cell list, everything but the pointers' values: counts, sizes, every cell's fields
// (a rectangle no larger than its crop, or with may_enlarge at least as large both ways, never one way only), and no
// two cells of one canvas that share a sample. No cell is read before cells and ncells are known to be good
static inline bool cells_ok(int cw, int ch, int ncanvas, int src_w, int src_h, int nsrc, const h264mi_cell *cells, int ncells, bool may_enlarge) {
    if (!cells || ncanvas <= 0 || nsrc <= 0 || ncells <= 0 || ncells > PIC_MAX_LIST || !sides_ok(cw, ch, src_w, src_h)) return false;
    for (int k = 0; k < ncells; k++) {
        const h264mi_cell &c = cells[k];
        if (c.src < 0 || c.src >= nsrc || c.canvas < 0 || c.canvas >= ncanvas) return false;
        if ((c.sx | c.sy | c.sw | c.sh | c.dx | c.dy | c.dw | c.dh) & 1) return false;
        if (c.sx < 0 || c.sy < 0 || c.sx > src_w || c.sy > src_h) return false;
        if (c.sw < 2 || c.sh < 2 || c.sw > src_w - c.sx || c.sh > src_h - c.sy) return false;  // sx <= src_w: no overflow
        if (c.dx < 0 || c.dy < 0 || c.dx > cw || c.dy > ch) return false;
        if (c.dw < 2 || c.dh < 2 || c.dw > cw - c.dx || c.dh > ch - c.dy) return false;
        const int kind = cell_kind(c);
        if (kind < 0 || (kind == 1 && !may_enlarge)) return false;
    }
    for (int k = 1; k < ncells; k++)
        for (int j = 0; j < k; j++) {
            const h264mi_cell &a = cells[k], &b = cells[j];
            if (a.canvas == b.canvas && rects_share(a.dx, a.dy, a.dw, a.dh, b.dx, b.dy, b.dw, b.dh)) return false;
        }
    return true;
}

// ---- cell tables
struct PictureCell {  // a cell as compose_kernel and upscale_kernel read it, 24 bytes
    int32_t src, canvas;
    uint16_t sx, sy, sw, sh, dx, dy, dw, dh;
};
static_assert(sizeof(PictureCell) == 24, "the launch structs count on it");
static inline PictureCell picture_cell(const h264mi_cell &c) {
    return PictureCell{c.src, c.canvas, (uint16_t)c.sx, (uint16_t)c.sy, (uint16_t)c.sw, (uint16_t)c.sh,
                       (uint16_t)c.dx, (uint16_t)c.dy, (uint16_t)c.dw, (uint16_t)c.dh};
}
// a launch's table: cell[k] from cells[k], and the prefix first[] of waves per cell (cell k's waves are first[k] ..
// first[k + 1] - 1; a cell has at most 128 * 512 + 2 * 64 * 256 waves, a launch 64 cells: far below 2^31). Returns n
static inline int fill_cell_table(PictureCell *cell, int *first, const h264mi_cell *cells, int n, int (*waves)(int dw, int dh)) {
    first[0] = 0;
    for (int k = 0; k < n; k++) {
        cell[k] = picture_cell(cells[k]);
        first[k + 1] = first[k] + waves(cells[k].dw, cells[k].dh);
    }
    return n;
}

// ---- layouts
// cell k of a layout: the largest picture of the whole source's shape in the slot X0..X1 x Y0..Y1 (no larger than the
// source unless may_enlarge), even sides, centred on even offsets, on canvas 0. false when a side falls below 2
static inline bool fit_centred(h264mi_cell *out, int k, int src_w, int src_h, int X0, int X1, int Y0, int Y1, bool may_enlarge) {
    const int cap_w = may_enlarge ? X1 - X0 : std::min(src_w, X1 - X0), cap_h = may_enlarge ? Y1 - Y0 : std::min(src_h, Y1 - Y0);
    const int dw = std::min(cap_w, 2 * ((Y1 - Y0) * src_w / (2 * src_h)));
    const int dh = std::min(cap_h, 2 * (dw * src_h / (2 * src_w)));
    if (dw < 2 || dh < 2) return false;
    *out = h264mi_cell{k, 0, 0, 0, src_w, src_h, X0 + 2 * ((X1 - X0 - dw) / 4), Y0 + 2 * ((Y1 - Y0 - dh) / 4), dw, dh};
    return true;
}
// arguments of a layout call: room for n cells, and the geometry
static inline bool layout_args_ok(const h264mi_cell *out, int cap, int n, int src_w, int src_h, int cw, int ch) {
    return out && n > 0 && n <= PIC_MAX_LIST && cap >= n && sides_ok(cw, ch, src_w, src_h);
}

// ---- what the code objects export to the runtime
// quality.hip
int launch_quality_enc(h264mi_quality *d_out, const uint8_t *d_frames, size_t fbytes, int w, int h, int cw, const EncDesc *desc, int S,
                       hipStream_t s);
int launch_quality_i420(h264mi_quality *d_out, const uint8_t *a, const uint8_t *b, int w, int h, int n, hipStream_t s);
bool quality_args_ok(int w, int h, int n);
// scale.hip
int launch_scale_i420(uint8_t *dst, int dw, int dh, const uint8_t *src, int sw, int sh, int n, hipStream_t s);
bool scale_args_ok(int dw, int dh, int sw, int sh, int n);
// compose.hip
int launch_compose_i420(uint8_t *dst, int cw, int ch, const uint8_t *src, int src_w, int src_h, const h264mi_cell *cells, int ncells,
                        hipStream_t s);
int launch_fill_i420(uint8_t *dst, int w, int h, int n, int y, int cb, int cr, hipStream_t s);
bool fill_args_ok(int w, int h, int n, int y, int cb, int cr);
int mosaic_cells(h264mi_cell *out, int cap, int n, int src_w, int src_h, int cw, int ch);
// overlay.hip
int launch_overlay_i420(uint8_t *dst, int cw, int ch, const uint8_t *spr, int ow, int oh, const h264mi_overlay *ov, int nov, hipStream_t s);
int launch_rgba_to_i420a(const uint8_t *d_rgba, int w, int h, int n, uint8_t *d_out, hipStream_t s);
bool overlay_args_ok(int cw, int ch, int ncanvas, int ow, int oh, int nsprites, const h264mi_overlay *ov, int nov);
int overlay_launch_end(const h264mi_overlay *ov, int nov, int k0);
bool rgba_to_i420a_args_ok(int w, int h, int n);
// upscale.hip
int launch_upscale_i420(uint8_t *dst, int dw, int dh, const uint8_t *src, int sw, int sh, int n, int filter, hipStream_t s);
bool upscale_args_ok(int dw, int dh, int sw, int sh, int n, int filter);
int launch_compose_any_i420(uint8_t *dst, int cw, int ch, const uint8_t *src, int src_w, int src_h, const h264mi_cell *cells, int ncells,
                            int filter, hipStream_t s);
int speaker_cells(h264mi_cell *out, int cap, int n, int speaker, int src_w, int src_h, int cw, int ch);
// orient.hip
int launch_orient_i420(uint8_t *dst, const uint8_t *src, int sw, int sh, int n, int orient, hipStream_t s);
bool orient_args_ok(int orient, int sw, int sh, int n);
int orient_size(int orient, int sw, int sh, int *dw, int *dh);
int orient_compose(int first, int then);
int orient_inverse(int orient);
void orient_plane_host(int orient, const uint8_t *S, int pw, int ph, uint8_t *D);
// denoise.hip: arguments as denoise_args_ok accepts them; stats: four words a frame, or null
int launch_denoise_i420(uint8_t *dst, uint8_t *dst2, const uint8_t *cur, const uint8_t *prev, int w, int h, int n, const h264mi_denoise &p,
                        uint32_t *stats, hipStream_t s);
void denoise_frame_host(uint8_t *out, const uint8_t *cur, const uint8_t *prev, int w, int h, const h264mi_denoise &p, uint32_t *stats);
// scenecut.hip: arguments as scenecut_args_ok accepts them; stats: eight words a frame, or null. scenecut_frame_host:
// one frame as plain loops, thumb_out (may be thumb_prev, or null) and stats (null without thumb_prev) as in the call
int launch_scenecut_i420(uint32_t *stats, uint8_t *thumb_out, const uint8_t *cur, const uint8_t *thumb_prev, int w, int h, int n,
                         const h264mi_scenecut &p, hipStream_t s);
void scenecut_frame_host(uint32_t *stats, uint8_t *thumb_out, const uint8_t *cur, const uint8_t *thumb_prev, int w, int h, const h264mi_scenecut &p);
// the decision of S streams, one thread each: st and words (16 a stream) on the device; stats eight words a stream
// on the device, or null (no detector ran: no thumbnail yet, or share == 0)
int launch_scenecut_decide(EncState *st, uint32_t *words, const uint32_t *stats, int S, const h264mi_scenecut &p, hipStream_t s);
// deinterlace.hip: arguments as deinterlace_args_ok accepts them; prev_out, prev and stats (four words a frame) may be
// null. deinterlace_frame_host: one frame sample by sample, out may be cur
int launch_deinterlace_i420(uint8_t *dst, uint8_t *prev_out, const uint8_t *cur, const uint8_t *prev, int w, int h, int n,
                            const h264mi_deinterlace &p, uint32_t *stats, hipStream_t s);
void deinterlace_frame_host(uint8_t *out, const uint8_t *cur, const uint8_t *prev, int w, int h, const h264mi_deinterlace &p, uint32_t *stats);
// spatial.hip: arguments as spatial_args_ok / privacy_ok accept them. The _host functions: the same rules as plain loops
int launch_spatial_i420(uint8_t *dst, const uint8_t *src, int w, int h, int n, const h264mi_spatial &p, hipStream_t s);
void spatial_frame_host(uint8_t *out, const uint8_t *src, int w, int h, const h264mi_spatial &p);
int launch_privacy_i420(uint8_t *frames, int w, int h, const h264mi_privacy *list, int nlist, hipStream_t s);
void privacy_frames_host(uint8_t *frames, int w, int h, const h264mi_privacy *list, int nlist);
// levels.hip: arguments as hist_args_ok / lut_args_ok / levels_args_ok accept them. The decide launch: hist null in FIXED
// mode, state and record may be null; luts receives n table sets. The _host functions: the same rules as plain loops
int launch_hist_i420(uint32_t *hist, const uint8_t *frames, int w, int h, int n, hipStream_t s);
int launch_lut_i420(uint8_t *dst, const uint8_t *src, int w, int h, int n, const uint8_t *luts, int per_frame, hipStream_t s);
int launch_levels_decide(uint8_t *luts, const uint32_t *hist, int32_t *state, int32_t *record, int w, int h, int n, const h264mi_levels &p,
                         hipStream_t s);
int launch_levels_i420(uint8_t *dst, const uint8_t *src, int w, int h, int n, const h264mi_levels &p, int32_t *state, int32_t *record,
                       uint8_t *work, hipStream_t s);
void hist_frame_host(uint32_t *hist, const uint8_t *frame, int w, int h);
void lut_frame_host(uint8_t *dst, const uint8_t *src, int w, int h, const uint8_t *lut768);
void levels_lut_host(uint8_t *lut768, const uint32_t *hist_y, int w, int h, const h264mi_levels &p, int32_t *state4, int32_t *record8);
// warp.hip: arguments as warp_args_ok accepts them; mesh on the device. warp_frame_host: one frame sample by sample,
// mesh on the host. The builders fill a host mesh and return its number of points, or -1. warp_tile_class: 0 when the
// kernel stages the source footprint of tile (tx, ty) of plane 0..2 in LDS, 1 when it samples global memory, -1 on a
// bad argument. path: 0, or 1 (measurement only) for the global path in every tile
int launch_warp_i420(uint8_t *dst, int dw, int dh, const uint8_t *src, int sw, int sh, int n, const int32_t *mesh, int mesh_per_frame,
                     const h264mi_warp &p, int path, hipStream_t s);
void warp_frame_host(uint8_t *dst, int dw, int dh, const uint8_t *src, int sw, int sh, const int32_t *mesh, const h264mi_warp &p);
int warp_mesh_affine(int32_t *mesh, int dw, int dh, int grid_log2, const int32_t *m6);
int warp_mesh_homography(int32_t *mesh, int dw, int dh, int grid_log2, const int32_t *h9);
int warp_mesh_radial(int32_t *mesh, int dw, int dh, int grid_log2, int cx, int cy, int64_t r2, int k1, int k2);
int warp_tile_class(const int32_t *mesh, int dw, int dh, int sw, int sh, int grid_log2, int plane, int tx, int ty);
// pixfmt.hip, pixdeep.hip
int launch_pix_to_i420(uint8_t *d_i420, const uint8_t *d_src, const h264mi_pix_layout &L, int w, int h, int n, hipStream_t s);
int launch_i420_to_pix(uint8_t *d_dst, const h264mi_pix_layout &L, const uint8_t *d_i420, int w, int h, int n, hipStream_t s);
int launch_pixdeep_to_i420(uint8_t *d_i420, const uint8_t *d_src, const h264mi_pix_layout &L, int depth, int w, int h, int n, hipStream_t s);
int launch_i420_to_pixdeep(uint8_t *d_dst, const h264mi_pix_layout &L, const uint8_t *d_i420, int w, int h, int n, hipStream_t s);
int launch_dec_output_pixdeep(int S, int cw, int ch, int w, int h, const DecDesc *desc, const DecInput *in, const h264mi_pix_layout &L,
                              hipStream_t s);
int launch_dec_output_pix(int S, int cw, int ch, int w, int h, const DecDesc *desc, const DecInput *in, const h264mi_pix_layout &L,
                          hipStream_t s);
// the two together: pixdeep.hip for its formats, pixfmt.hip (which reads no depth rule) for the others
static inline int launch_layout_to_i420(uint8_t *d_i420, const uint8_t *d_src, const h264mi_pix_layout &L, int depth, int w, int h, int n,
                                        hipStream_t s) {
    return pix_is_deep(L.pix) ? launch_pixdeep_to_i420(d_i420, d_src, L, depth, w, h, n, s) : launch_pix_to_i420(d_i420, d_src, L, w, h, n, s);
}
static inline int launch_i420_to_layout(uint8_t *d_dst, const h264mi_pix_layout &L, const uint8_t *d_i420, int w, int h, int n, hipStream_t s) {
    return pix_is_deep(L.pix) ? launch_i420_to_pixdeep(d_dst, L, d_i420, w, h, n, s) : launch_i420_to_pix(d_dst, L, d_i420, w, h, n, s);
}
static inline int launch_dec_output_layout(int S, int cw, int ch, int w, int h, const DecDesc *desc, const DecInput *in,
                                           const h264mi_pix_layout &L, hipStream_t s) {
    return pix_is_deep(L.pix) ? launch_dec_output_pixdeep(S, cw, ch, w, h, desc, in, L, s) : launch_dec_output_pix(S, cw, ch, w, h, desc, in, L, s);
}
// colorspace.hip: a good specification, even sides within PIC_MAX_SIDE; alpha: I420A sprites out (A = the fourth byte)
int launch_rgba_to_i420_cs(uint8_t *d_out, const uint8_t *d_rgba, int w, int h, int n, const h264mi_colorspec &spec, bool alpha, hipStream_t s);
int launch_i420_to_rgba_cs(uint8_t *d_rgba, const uint8_t *d_i420, int w, int h, int n, const h264mi_colorspec &spec, hipStream_t s);
int launch_dec_output_rgba_cs(int S, int cw, int ch, const DecDesc *desc, const DecInput *in, const h264mi_colorspec &spec, hipStream_t s);
}  // namespace h264mi
