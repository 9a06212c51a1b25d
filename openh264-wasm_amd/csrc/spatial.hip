// spatial.hip -- the spatial filter (unsharp mask / blur) and the privacy masks of tight I420 frames on the device
// (gfx950), as include/h264mi.h defines them (h264mi_i420_spatial_dev, h264mi_i420_privacy_dev). DESIGN.md §5.18.
//   spatial_kernel : n frames of one geometry per launch -- the standalone call, or an encoder's input area filtered
//                    into the stage's own frames (h264mi_enc_set_spatial)
//   privacy_kernel : up to H264MI_PRIVACY_PER_LAUNCH rectangles per launch, in place -- the standalone call, or an
//                    encoder's list (h264mi_enc_set_privacy)
// The filter, per plane with the radius r and the amount of its kind: L is the separable binomial of radius r over
// clamped coordinates, rounded once, L = (S + (1 << (4r - 1))) >> 4r; d = C - L; amount > 0 and |d| <= core keep C, else
// O = clip(C + ((amount d + 32) >> 6)). picture_host.h holds the weights and the sample rule for host and device.
//
// Work split. A block of four waves owns one tile -- SP_TW = 256 samples by SP_TH = 32 rows of one plane of one frame.
// The items (frame, plane, tile row, tile) are dealt to at most PIC_MAX_BLOCKS blocks in runs of consecutive items; the
// loop count and every branch around a barrier depend on the block only. A tile of a plane that is copied (r == 0 or
// amount == 0) is moved row by row, no LDS. A filtered tile takes three steps with a barrier behind each:
//   load:  rows y0 - r .. y0 + th - 1 + r (row numbers clamped to the plane) of columns x0 .. x0 + tw - 1 into sb[][],
//          a wave a row, a lane a dword; then the 2r halo bytes of each row, columns clamped to the plane, a thread a
//          byte. Clamping happens here and nowhere else: the two passes see a tile with a full border.
//   rows:  the horizontal sums into hs[][] as 16-bit words (at most 255 * 64). A thread takes four neighbouring columns
//          of one row: three aligned dwords of sb, v_perm_b32 picks the byte pairs (x, x + 1) and (x + 2, x + 3) of each
//          tap into the halves of a register, and the weighted sums of a pair are packed 16-bit multiply-adds.
//   cols:  a thread takes four columns of eight rows: the 8 + 2r rows of hs it needs are read once (ds_read_b64), the
//          2-D sum is formed in 32 bits, rounded, the sample rule applied to the centre bytes of sb, and a dword stored:
//          a wave stores 256 consecutive bytes of a row.
// Two paths for the same bytes, chosen per plane and frame from the plane's own pointers and row length: a plane whose
// two bases and row length are multiples of 4 moves as dwords; any other plane (a buffer at an odd address, a chroma
// row of 18 bytes) moves as bytes into and out of the same LDS layout. An aligned dword of a row whose length is a
// multiple of 4 never leaves the row, the byte path tests every column: no access leaves a plane.
// Out of place only: a tile reads rows and columns that its neighbours write.
//
// Pixelate: a wave owns one cell of one plane of one rectangle. The launch's arguments hold the rectangles and a prefix
// table of waves per rectangle (overlay.hip's scheme). The lanes read the cell (64 / cw rows at a time), the sum meets
// in a butterfly of the wave (picture_dev.h's wave_sum), and every lane stores the mean to the samples it read: a cell reads only what it writes,
// so in place needs no scratch and no order. FILL is the same walk with 64 x 64 cells, no read and the fill value.
//
// A translation unit and a code object of its own, as denoise.hip is: the library's other kernels stay byte for byte
// what they were. The host runtime (enc_input.inc, capi_enc.inc) reaches it through the functions picture_host.h declares.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/h264mi.h"
#include "picture_host.h"
#include "picture_dev.h"

namespace h264mi {
#define SP_TW 256                   // samples across a tile
#define SP_TH 32                    // rows of a tile
#define SP_ROWS (SP_TH + 2 * 3)     // with the halo rows of the largest radius
#define SP_LEAD 8                   // bytes in front of a tile row in sb: the left halo, dword-aligned interior
#define SP_PITCH (SP_LEAD + SP_TW + 8)

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

struct SpatialLaunch {
    const uint8_t *src;
    uint8_t *dst;
    size_t fb;             // frame f of each: base + f * fb
    size_t off[3];         // a frame's planes
    int w, h;
    int r[2], amount[2];   // luma, chroma
    int core;
    int ntx[2], nty[2];    // tiles across and down a plane of each kind
    int per_frame;         // ntx[0] nty[0] + 2 ntx[1] nty[1]
    long long items, per;  // n * per_frame; items a block
};

PICDEV int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// the bytes o and o + 1 (o = 1..9) of the twelve bytes d0 d1 d2 in the low bytes of the two halves of a register
PICDEV us2 byte_pair(uint32_t d0, uint32_t d1, uint32_t d2, int o) {
    const int j = o >> 2, b = o & 3;
    const uint32_t lo = j == 0 ? d0 : j == 1 ? d1 : d2, hi = j == 0 ? d1 : j == 1 ? d2 : 0u;
    const uint32_t sel = (uint32_t)b | 0x0c00u | ((uint32_t)(b + 1) << 16) | 0x0c000000u;
    return __builtin_bit_cast(us2, __builtin_amdgcn_perm(hi, lo, sel));
}

PICDEV void copy_tile(const uint8_t *S, uint8_t *D, int pw, int x0, int y0, int tw, int th, bool wide, int t) {
    const int c = 4 * (t & 63);
    if (c >= tw) return;
    for (int i = t >> 6; i < th; i += 4) {
        const size_t o = (size_t)(y0 + i) * pw + x0 + c;
        if (wide) {
            *(uint32_t *)(D + o) = *(const uint32_t *)(S + o);
        } else {
            for (int j = 0; j < 4 && c + j < tw; j++) D[o + j] = S[o + j];
        }
    }
}

template <int R>
PICDEV void filter_tile(uint8_t (*sb)[SP_PITCH], uint16_t (*hs)[SP_TW], const uint8_t *S, uint8_t *D, int pw, int ph, int x0, int y0, int tw,
                      int th, bool wide, int amount, int core, int t) {
    const int q = t & 63, wv = t >> 6, c = 4 * q;
    const int nrows = th + 2 * R;
    // ---- load: the tile's rows, then their halo bytes
    if (c < tw)
        for (int i = wv; i < nrows; i += 4) {
            const uint8_t *row = S + (size_t)clampi(y0 - R + i, 0, ph - 1) * pw + x0;
            if (wide) {
                *(uint32_t *)&sb[i][SP_LEAD + c] = *(const uint32_t *)(row + c);
            } else {
                for (int j = 0; j < 4 && c + j < tw; j++) sb[i][SP_LEAD + c + j] = row[c + j];
            }
        }
    for (int k = t; k < nrows * 2 * R; k += 256) {
        const int i = k / (2 * R), j = k - i * 2 * R;
        const int hc = j < R ? j - R : tw + j - R;  // -R .. -1, tw .. tw + R - 1
        sb[i][SP_LEAD + hc] = S[(size_t)clampi(y0 - R + i, 0, ph - 1) * pw + clampi(x0 + hc, 0, pw - 1)];
    }
    __syncthreads();
    // ---- rows: four horizontal sums a thread
    if (c < tw)
        for (int i = wv; i < nrows; i += 4) {
            const uint32_t *p = (const uint32_t *)&sb[i][SP_LEAD + c - 4];  // the bytes of columns c - 4 .. c + 7
            const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];
            us2 lo = {0, 0}, hi = {0, 0};
#pragma unroll
            for (int k = 0; k <= 2 * R; k++) {
                const unsigned short wt = (unsigned short)spatial_weight(R, k);
                const us2 w2 = {wt, wt};
                lo += w2 * byte_pair(d0, d1, d2, 4 - R + k);
                hi += w2 * byte_pair(d0, d1, d2, 6 - R + k);
            }
            *(uint2 *)&hs[i][c] = make_uint2(__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi));
        }
    __syncthreads();
    // ---- cols: four columns of eight rows a thread
    const int r0 = 8 * wv;
    if (c < tw && r0 < th) {
        uint2 win[8 + 2 * R];
#pragma unroll
        for (int k = 0; k < 8 + 2 * R; k++) win[k] = *(const uint2 *)&hs[r0 + k][c];  // r0 + k < SP_ROWS; rows from nrows on feed no stored row
#pragma unroll
        for (int rr = 0; rr < 8; rr++) {
            if (r0 + rr < th) {
                uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
                for (int k = 0; k <= 2 * R; k++) {
                    const uint32_t wt = (uint32_t)spatial_weight(R, k);
                    s0 += wt * (win[rr + k].x & 0xffffu); s1 += wt * (win[rr + k].x >> 16);
                    s2 += wt * (win[rr + k].y & 0xffffu); s3 += wt * (win[rr + k].y >> 16);
                }
                const uint32_t c4 = *(const uint32_t *)&sb[r0 + rr + R][SP_LEAD + c];
                const uint32_t rnd = 1u << (4 * R - 1);
                const uint32_t o0 = (uint32_t)spatial_sample((int)(c4 & 255u), (int)((s0 + rnd) >> (4 * R)), amount, core);
                const uint32_t o1 = (uint32_t)spatial_sample((int)((c4 >> 8) & 255u), (int)((s1 + rnd) >> (4 * R)), amount, core);
                const uint32_t o2 = (uint32_t)spatial_sample((int)((c4 >> 16) & 255u), (int)((s2 + rnd) >> (4 * R)), amount, core);
                const uint32_t o3 = (uint32_t)spatial_sample((int)(c4 >> 24), (int)((s3 + rnd) >> (4 * R)), amount, core);
                const uint32_t o4 = o0 | (o1 << 8) | (o2 << 16) | (o3 << 24);
                const size_t o = (size_t)(y0 + r0 + rr) * pw + x0 + c;
                if (wide) {
                    *(uint32_t *)(D + o) = o4;
                } else {
                    for (int j = 0; j < 4 && c + j < tw; j++) D[o + j] = (uint8_t)(o4 >> (8 * j));
                }
            }
        }
    }
    __syncthreads();  // the next item's load writes sb and hs
}

__global__ __launch_bounds__(256) void spatial_kernel(SpatialLaunch a) {
    __shared__ __attribute__((aligned(16))) uint8_t sb[SP_ROWS][SP_PITCH];
    __shared__ __attribute__((aligned(16))) uint16_t hs[SP_ROWS][SP_TW];
    const int t = threadIdx.x;
    const long long it0 = (long long)blockIdx.x * a.per, it1 = min(it0 + a.per, a.items);
    const int n_y = a.ntx[0] * a.nty[0], n_c = a.ntx[1] * a.nty[1];
    for (long long it = it0; it < it1; it++) {  // the same count, plane and radius in every thread of a block
        const long long f = it / a.per_frame;
        int k = (int)(it - f * a.per_frame), pl = 0;
        if (k >= n_y) { k -= n_y; pl = 1 + k / n_c; k -= (pl - 1) * n_c; }
        const int kind = pl ? 1 : 0;
        const int ty = k / a.ntx[kind], tx = k - ty * a.ntx[kind];
        const int pw = pl ? a.w >> 1 : a.w, ph = pl ? a.h >> 1 : a.h;
        const int x0 = tx * SP_TW, y0 = ty * SP_TH;
        const int tw = min(SP_TW, pw - x0), th = min(SP_TH, ph - y0);
        const uint8_t *S = a.src + (size_t)f * a.fb + a.off[pl];
        uint8_t *D = a.dst + (size_t)f * a.fb + a.off[pl];
        const bool wide = ((((uintptr_t)S) | ((uintptr_t)D) | (uintptr_t)pw) & 3) == 0;  // then tw is a multiple of 4
        const int r = a.r[kind], amount = a.amount[kind];
        if (r == 0 || amount == 0) copy_tile(S, D, pw, x0, y0, tw, th, wide, t);
        else if (r == 1) filter_tile<1>(sb, hs, S, D, pw, ph, x0, y0, tw, th, wide, amount, a.core, t);
        else if (r == 2) filter_tile<2>(sb, hs, S, D, pw, ph, x0, y0, tw, th, wide, amount, a.core, t);
        else filter_tile<3>(sb, hs, S, D, pw, ph, x0, y0, tw, th, wide, amount, a.core, t);
    }
}

// ---- privacy masks
struct PrivacyItem {  // a rectangle as the kernel reads it, 20 bytes of whole words
    int32_t frame;
    uint32_t xy, wh;  // x | y << 16, w | h << 16
    uint32_t walk;    // bit 0: FILL; bits 8..15: the luma cell side of the walk
    uint32_t fill;    // fill_y | fill_cb << 8 | fill_cr << 16
};
struct PrivacyLaunch {
    uint8_t *frames;
    size_t fb;
    int w, h, n;
    int first[H264MI_PRIVACY_PER_LAUNCH + 1];  // rectangle k's waves are first[k] .. first[k + 1] - 1
    PrivacyItem item[H264MI_PRIVACY_PER_LAUNCH];
};
static_assert(sizeof(PrivacyLaunch) < 2048, "the argument block stays well below 4 KB");

// the cell side a rectangle is walked with, and its waves: three planes of cells
static inline int privacy_side(const h264mi_privacy &m) { return m.mode == H264MI_PRIVACY_FILL ? 64 : m.block; }
static inline int privacy_waves(const h264mi_privacy &m) {
    const int B = privacy_side(m);
    return 3 * ((m.w + B - 1) / B) * ((m.h + B - 1) / B);
}

__global__ __launch_bounds__(256) void privacy_kernel(PrivacyLaunch a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int items = a.first[a.n];
    for (int it = (int)blockIdx.x * 4 + wave; it < items; it += (int)gridDim.x * 4) {
        int lo_c = 0, hi_c = a.n;  // first[lo_c] <= it < first[hi_c]
        while (hi_c - lo_c > 1) {
            const int mid_c = (lo_c + hi_c) >> 1;
            if (a.first[mid_c] <= it) lo_c = mid_c; else hi_c = mid_c;
        }
        const PrivacyItem m = a.item[lo_c];
        const bool fill = m.walk & 1;
        const int B = (int)(m.walk >> 8);
        const int mx = (int)(m.xy & 0xffffu), my = (int)(m.xy >> 16), mw = (int)(m.wh & 0xffffu), mh = (int)(m.wh >> 16);
        const int ncx = (mw + B - 1) / B, ncy = (mh + B - 1) / B, ncell = ncx * ncy;
        int k = it - a.first[lo_c];
        const int pl = k / ncell;
        k -= pl * ncell;
        const int cy = k / ncx, cx = k - cy * ncx;
        const int sh = pl ? 1 : 0, Bp = B >> sh;                      // the plane's cell side
        const int pw = a.w >> sh, rw = mw >> sh, rh = mh >> sh;     // the plane's row length, the rectangle in it
        const int cw = min(Bp, rw - cx * Bp), ch = min(Bp, rh - cy * Bp);  // the cell: 1 .. 64 each way
        const size_t poff = pl == 0 ? 0 : (size_t)a.w * a.h + (pl == 2 ? (size_t)(a.w >> 1) * (a.h >> 1) : 0);
        uint8_t *P = a.frames + (size_t)m.frame * a.fb + poff + (size_t)((my >> sh) + cy * Bp) * pw + (mx >> sh) + cx * Bp;
        const int rp = 64 / cw;                      // rows a pass
        const int ly = lane / cw, lx = lane - ly * cw;
        const bool on = ly < rp;
        uint32_t v;
        if (fill) {
            v = (m.fill >> (8 * pl)) & 255u;
        } else {
            uint32_t sum = 0;
            if (on)
                for (int y = ly; y < ch; y += rp) sum += P[(size_t)y * pw + lx];
            const uint32_t n = (uint32_t)(cw * ch);
            v = (wave_sum(sum) + n / 2) / n;         // the stores below depend on every load of the cell
        }
        if (on)
            for (int y = ly; y < ch; y += rp) P[(size_t)y * pw + lx] = (uint8_t)v;
    }
}

// ---- host
// the definitions on the host as plain loops. spatial: one frame, out and src tight w x h frames that share no byte
void spatial_frame_host(uint8_t *out, const uint8_t *src, int w, int h, const h264mi_spatial &p) {
    const size_t off[3] = {0, (size_t)w * h, (size_t)w * h + (size_t)(w / 2) * (h / 2)};
    for (int pl = 0; pl < 3; pl++) {
        const int pw = pl ? w / 2 : w, ph = pl ? h / 2 : h;
        const int r = pl ? p.radius_c : p.radius_y, amount = pl ? p.amount_c : p.amount_y;
        const uint8_t *S = src + off[pl];
        uint8_t *O = out + off[pl];
        for (int y = 0; y < ph; y++)
            for (int x = 0; x < pw; x++) {
                const int c = S[(size_t)y * pw + x];
                if (r == 0) { O[(size_t)y * pw + x] = (uint8_t)c; continue; }
                int sum = 0;
                for (int j = -r; j <= r; j++)
                    for (int i = -r; i <= r; i++) {
                        const int yy = std::min(std::max(y + j, 0), ph - 1), xx = std::min(std::max(x + i, 0), pw - 1);
                        sum += spatial_weight(r, j + r) * spatial_weight(r, i + r) * S[(size_t)yy * pw + xx];
                    }
                const int l = (sum + (1 << (4 * r - 1))) >> (4 * r);
                O[(size_t)y * pw + x] = (uint8_t)spatial_sample(c, l, amount, p.core);
            }
    }
}
// privacy: the frames of a call in place; list as privacy_ok accepts it
void privacy_frames_host(uint8_t *frames, int w, int h, const h264mi_privacy *list, int nlist) {
    const size_t fb = i420_bytes(w, h);
    const size_t off[3] = {0, (size_t)w * h, (size_t)w * h + (size_t)(w / 2) * (h / 2)};
    for (int k = 0; k < nlist; k++) {
        const h264mi_privacy &m = list[k];
        for (int pl = 0; pl < 3; pl++) {
            const int sh = pl ? 1 : 0, pw = w >> sh;
            const int rx = m.x >> sh, ry = m.y >> sh, rw = m.w >> sh, rh = m.h >> sh;
            uint8_t *P = frames + (size_t)m.frame * fb + off[pl];
            if (m.mode == H264MI_PRIVACY_FILL) {
                const uint8_t v = (uint8_t)(pl == 0 ? m.fill_y : pl == 1 ? m.fill_cb : m.fill_cr);
                for (int y = 0; y < rh; y++)
                    for (int x = 0; x < rw; x++) P[(size_t)(ry + y) * pw + rx + x] = v;
                continue;
            }
            const int B = m.block >> sh;
            for (int cy = 0; cy * B < rh; cy++)
                for (int cx = 0; cx * B < rw; cx++) {
                    const int cw = std::min(B, rw - cx * B), ch = std::min(B, rh - cy * B);
                    uint32_t sum = 0;
                    for (int y = 0; y < ch; y++)
                        for (int x = 0; x < cw; x++) sum += P[(size_t)(ry + cy * B + y) * pw + rx + cx * B + x];
                    const uint32_t n = (uint32_t)(cw * ch);
                    const uint8_t v = (uint8_t)((sum + n / 2) / n);
                    for (int y = 0; y < ch; y++)
                        for (int x = 0; x < cw; x++) P[(size_t)(ry + cy * B + y) * pw + rx + cx * B + x] = v;
                }
        }
    }
}

// n tight w x h I420 frames: arguments as spatial_args_ok accepts them. One launch
int launch_spatial_i420(uint8_t *dst, const uint8_t *src, int w, int h, int n, const h264mi_spatial &p, hipStream_t s) {
    const size_t ly = (size_t)w * h, lc = (size_t)(w / 2) * (h / 2);
    SpatialLaunch a{};
    a.src = src; a.dst = dst;
    a.fb = ly + 2 * lc;
    a.off[0] = 0; a.off[1] = ly; a.off[2] = ly + lc;
    a.w = w; a.h = h;
    a.r[0] = p.radius_y; a.r[1] = p.radius_c; a.amount[0] = p.amount_y; a.amount[1] = p.amount_c; a.core = p.core;
    for (int k = 0; k < 2; k++) {
        a.ntx[k] = ((w >> k) + SP_TW - 1) / SP_TW;
        a.nty[k] = ((h >> k) + SP_TH - 1) / SP_TH;
    }
    a.per_frame = a.ntx[0] * a.nty[0] + 2 * a.ntx[1] * a.nty[1];
    a.items = (long long)n * a.per_frame;
    const long long blocks = std::min(a.items, (long long)PIC_MAX_BLOCKS);
    a.per = (a.items + blocks - 1) / blocks;
    (void)hipGetLastError();
    hipLaunchKernelGGL(spatial_kernel, dim3((unsigned)((a.items + a.per - 1) / a.per)), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// the frames of a call in place: a list as privacy_ok accepts it. One launch per H264MI_PRIVACY_PER_LAUNCH entries; no two
// entries share a sample, so neither the launches nor the waves of one need an order
int launch_privacy_i420(uint8_t *frames, int w, int h, const h264mi_privacy *list, int nlist, hipStream_t s) {
    for (int k0 = 0; k0 < nlist; k0 += H264MI_PRIVACY_PER_LAUNCH) {
        PrivacyLaunch a{};
        a.frames = frames; a.fb = i420_bytes(w, h); a.w = w; a.h = h;
        a.n = std::min(H264MI_PRIVACY_PER_LAUNCH, nlist - k0);
        a.first[0] = 0;
        for (int k = 0; k < a.n; k++) {
            const h264mi_privacy &m = list[k0 + k];
            const bool fill = m.mode == H264MI_PRIVACY_FILL;
            a.item[k] = PrivacyItem{m.frame, (uint32_t)m.x | (uint32_t)m.y << 16, (uint32_t)m.w | (uint32_t)m.h << 16,
                                    (fill ? 1u : 0u) | (uint32_t)privacy_side(m) << 8,
                                    fill ? (uint32_t)m.fill_y | (uint32_t)m.fill_cb << 8 | (uint32_t)m.fill_cr << 16 : 0u};
            a.first[k + 1] = a.first[k] + privacy_waves(m);  // at most 3 * 2048^2 a rectangle, 64 rectangles: below 2^31
        }
        (void)hipGetLastError();
        hipLaunchKernelGGL(privacy_kernel, dim3(launch_blocks(a.first[a.n])), dim3(256), 0, s, a);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}
}  // namespace h264mi
