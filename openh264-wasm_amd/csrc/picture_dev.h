// picture_dev.h -- the device half that the picture code objects share, included by the picture .hip files only, after
// picture_host.h: the inline macro, the wave's sums and counters, the four-lane dword store of a row segment
// (scale.hip, compose.hip, upscale.hip, overlay.hip) and the area average of scale.hip and compose.hip. Everything is
// inlined into the including unit: the units stay a code object each. DESIGN.md §5.8.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace h264mi {
#define PICDEV __device__ __forceinline__

// ---- sums over the 64 lanes, every lane running
PICDEV uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the counters c... summed over the wave; lane 0 adds the non-zero sums to st[0], st[1], .. (one atomic a wave and word)
PICDEV void add_nonzero(uint32_t *) {}
template <class... T>
PICDEV void add_nonzero(uint32_t *st, uint32_t v, T... rest) {
    if (v) atomicAdd(st, v);
    add_nonzero(st + 1, rest...);
}
template <class... T>
PICDEV void lane0_add_nonzero(uint32_t *st, int lane, T... v) {
    if (lane == 0) add_nonzero(st, v...);
}
template <class... T>
PICDEV void wave_add_counters(uint32_t *st, int lane, T... c) { lane0_add_nonzero(st, lane, wave_sum(c)...); }  // the sums first, in every lane

// ---- a row segment of n samples at p, sample i a lane, stored as dwords where it can be
// q: in lanes whose i is a multiple of 4, the samples of i .. i + 3. Every lane runs it
PICDEV uint32_t seg_pack(uint32_t v) {
    uint32_t q = v | (__shfl_down(v, 1) << 8);
    q |= __shfl_down(q, 2) << 16;
    return q;
}
// sample i < n: with p a multiple of 4, a group of four that lies inside the segment is one dword store of its first
// lane; a segment's last samples past such a group, and every sample of a segment at any other address, are bytes
PICDEV void seg_store(uint8_t *p, int i, int n, uint32_t v, uint32_t q) {
    if (i < n) {
        if ((((uintptr_t)p) & 3) == 0 && (i | 3) < n) { if ((i & 3) == 0) *(uint32_t *)(p + i) = q; }
        else p[i] = (uint8_t)v;
    }
}
// both for a p that is the same in every lane (a wave's row of 64 columns): no shuffle for a row that goes as bytes
PICDEV void seg_put(uint8_t *p, int i, int n, uint32_t v) {
    if ((((uintptr_t)p) & 3) == 0) seg_store(p, i, n, v, seg_pack(v));
    else if (i < n) p[i] = (uint8_t)v;
}

// ---- the area average (scale.hip's header has the formula). A wave owns a strip of 64 output columns and a segment of
// PIC_AREA_ROWS output rows of a pw x ph crop averaged to a qw x qh rectangle, a lane per output column
#define PIC_AREA_ROWS 16          // output rows per wave
#define PIC_AREA_BATCH 8          // source rows whose loads are in flight together
__host__ __device__ static inline int area_nstrip(int qw) { return (qw + 63) / 64; }
__host__ __device__ static inline int area_nseg(int qh) { return (qh + PIC_AREA_ROWS - 1) / PIC_AREA_ROWS; }

// the taps of output column ox: columns i0..i1 of the plane row (x0: the crop's first), weights wf, qw, .., qw, wl
struct AreaTaps { int i0, i1; uint32_t wf, wl; };
PICDEV AreaTaps area_taps(bool act, int ox, int pw, int qw, int x0) {
    AreaTaps t{x0, x0, 0, 0};
    if (act) {
        const int lo = ox * pw, hi = lo + pw;  // the output column in units of 1 / (pw qw)
        const int t0 = lo / qw, t1 = (hi + qw - 1) / qw - 1;
        t.wf = (uint32_t)(min((t0 + 1) * qw, hi) - lo);
        t.wl = t1 > t0 ? (uint32_t)(hi - t1 * qw) : 0u;
        t.i0 = x0 + t0;
        t.i1 = x0 + t1;
    }
    return t;
}
// the horizontal sums of one output column on PIC_AREA_BATCH plane rows (row r at byte S + row[r]): wf p[i0] + qw
// (p[i0+1] + .. + p[i1-1]) + wl p[i1] each (wl = 0 when i1 == i0), from byte loads. The rows' loads of one tap are
// independent of each other and issued together.
PICDEV void area_hsum_bytes(uint32_t *h, const uint8_t *S, const uint32_t *row, const AreaTaps &t, uint32_t qw) {
    uint32_t mid[PIC_AREA_BATCH];
#pragma unroll
    for (int r = 0; r < PIC_AREA_BATCH; r++) mid[r] = 0;
    for (int i = t.i0 + 1; i < t.i1; i++) {
#pragma unroll
        for (int r = 0; r < PIC_AREA_BATCH; r++) mid[r] += S[row[r] + i];
    }
#pragma unroll
    for (int r = 0; r < PIC_AREA_BATCH; r++) h[r] = t.wf * S[row[r] + t.i0] + qw * mid[r] + t.wl * S[row[r] + t.i1];
}
// the same from the aligned dwords i0 / 4 .. i1 / 4 of plane rows that start at a multiple of 4 and are a multiple of
// 4 long: the taps between the first and the last are summed by v_sad_u8 under a byte mask, which the rows share.
// Bytes of those dwords below i0 or above i1 (outside the crop, inside the row) are under no mask and in no shift.
PICDEV void area_hsum_dwords(uint32_t *h, const uint8_t *S, const uint32_t *row, const AreaTaps &t, uint32_t qw) {
    const int i0 = t.i0, i1 = t.i1, d0 = i0 >> 2, d1 = i1 >> 2;
    uint32_t mid[PIC_AREA_BATCH], first[PIC_AREA_BATCH], last[PIC_AREA_BATCH];
#pragma unroll
    for (int r = 0; r < PIC_AREA_BATCH; r++) mid[r] = first[r] = last[r] = 0;
    for (int d = d0; d <= d1; d++) {
        uint32_t v[PIC_AREA_BATCH];
#pragma unroll
        for (int r = 0; r < PIC_AREA_BATCH; r++) v[r] = *(const uint32_t *)(S + row[r] + 4 * d);
        const int lo = max(i0 + 1 - 4 * d, 0), hi = min(i1 - 1 - 4 * d, 3);  // the dword's bytes between the end taps
        const uint32_t m = lo <= hi ? (0xffffffffu >> (8 * (3 - hi))) & (0xffffffffu << (8 * lo)) : 0u;
#pragma unroll
        for (int r = 0; r < PIC_AREA_BATCH; r++) {
            mid[r] = __builtin_amdgcn_sad_u8(v[r] & m, 0u, mid[r]);
            if (d == d0) first[r] = (v[r] >> (8 * (i0 & 3))) & 255u;
            if (d == d1) last[r] = (v[r] >> (8 * (i1 & 3))) & 255u;
        }
    }
#pragma unroll
    for (int r = 0; r < PIC_AREA_BATCH; r++) h[r] = t.wf * first[r] + qw * mid[r] + t.wl * last[r];
}
// strip `strip`, segment `seg` of the rectangle at D (pitch dpitch) from the crop whose first row is at S (pitch
// spitch) and whose first column is x0; wide: the source plane's base and spitch are multiples of 4. The overlapping
// crop rows are walked downward a batch at a time: its horizontal sums, then the rows in order, each added under its
// vertical weight; an output row is stored once its last source row has gone by
PICDEV void area_average(uint8_t *D, int dpitch, const uint8_t *S, int spitch, bool wide, int x0, int pw, int ph, int qw, int qh, int strip,
                         int seg, int lane) {
    const int ox = strip * 64 + lane;
    const bool act = ox < qw;
    const AreaTaps t = area_taps(act, ox, pw, qw, x0);
    const uint32_t area = (uint32_t)pw * (uint32_t)ph, half = area >> 1;
    const int oy0 = seg * PIC_AREA_ROWS, oy1 = min(oy0 + PIC_AREA_ROWS, qh);
    const int y0 = (oy0 * ph) / qh, y1 = (oy1 * ph + qh - 1) / qh - 1;  // crop rows y0..y1
    int oy = oy0;
    uint32_t acc = 0;
    for (int yb0 = y0; yb0 <= y1; yb0 += PIC_AREA_BATCH) {
        uint32_t hs[PIC_AREA_BATCH];
#pragma unroll
        for (int r = 0; r < PIC_AREA_BATCH; r++) hs[r] = 0;
        if (act) {
            uint32_t row[PIC_AREA_BATCH];  // byte offsets from S; rows beyond y1 read row y1 again and are not used
#pragma unroll
            for (int r = 0; r < PIC_AREA_BATCH; r++) row[r] = (uint32_t)(min(yb0 + r, y1) * spitch);
            if (wide) area_hsum_dwords(hs, S, row, t, (uint32_t)qw);
            else area_hsum_bytes(hs, S, row, t, (uint32_t)qw);
        }
#pragma unroll
        for (int r = 0; r < PIC_AREA_BATCH; r++) {
            const int y = yb0 + r;
            if (y > y1) break;
            const uint32_t h = hs[r];
            const int top = oy * ph, bot = top + ph, ya = y * qh, yb = ya + qh;  // the same in every lane
            acc += (uint32_t)(min(yb, bot) - max(ya, top)) * h;
            if (yb >= bot) {  // output row oy is complete
                seg_put(D + (size_t)oy * dpitch + strip * 64, lane, qw - strip * 64, (acc + half) / area);
                oy++;
                acc = (uint32_t)(yb - bot) * h;  // the rest of a straddling row opens the next one
            }
        }
    }
}
}  // namespace h264mi
