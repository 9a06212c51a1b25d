// scale.hip -- area-average downscaling of tight I420 frames on the device (gfx950), as include/h264mi.h
// (h264mi_i420_scale_dev) defines it. DESIGN.md §5.3.
//   scale_kernel : n frames of one geometry pair per launch -- the standalone call, or an encoder's source frames
//                  scaled into its input area (h264mi_enc_encode_scaled)
// Every plane is scaled on its own (Y sw x sh -> dw x dh; Cb, Cr sw/2 x sh/2 -> dw/2 x dh/2). For a plane of
// pw x ph samples scaled to qw x qh, source column i weighs max(0, min((i+1) qw, (ox+1) pw) - max(i qw, ox pw)) in
// output column ox, rows likewise with ph, qh, and out = (sum wy wx p + (pw ph >> 1)) / (pw ph). The sum is
// separable, every partial is an integer, and with pw, ph <= 4096 the numerator stays below 2^32: unsigned 32-bit
// accumulation is exact and the result does not depend on the order of evaluation.
// A wave owns a strip of 64 output columns and a segment of H264MI_SCALE_ROWS output rows of one plane of one
// frame and walks the overlapping source rows downward: per source row a lane forms the horizontal sum of its
// output column (its taps i0..i1 and their weights are the same on every row: the first and last tap weigh wf and
// wl, every tap between them qw), adds wy times it to the accumulator of the current output row and, when the
// source row straddles two output rows, starts the next row's accumulator with the rest. An output row is stored
// once its last source row has gone by, so inside a strip segment a source sample is loaded once (adjacent strips
// share at most one column, adjacent segments one row). The taps are a loop: 1 to ceil(pw / qw) + 1 of them.
// The source rows are taken H264MI_SCALE_BATCH at a time: the horizontal sums of a batch are formed together, so
// that a tap's loads of all its rows are in flight at once (one row at a time the walk is a chain of dependent
// loads and runs at memory latency), then the rows are added in order.
// A source plane whose rows can be read as dwords (base address and pw multiples of 4) is read as the aligned
// dwords that hold the taps -- the taps between the first and the last are summed by v_sad_u8 under a byte mask --;
// any other (w % 8 != 0 chroma, a buffer at an odd address) is read byte by byte. An output row segment that
// starts at a multiple of 4 is stored as dwords gathered from four lanes, any other (and a strip's last columns)
// as bytes. The same bytes either way; the tests are per plane and frame, from the plane's own pointers. An
// aligned dword of a row whose length is a multiple of 4 never leaves the row: no access leaves the pw x ph area
// of the source plane or the qw x qh area of the destination plane.
//
// A translation unit and a code object of its own, as quality.hip is: the library's other kernels stay byte for
// byte what they were. The host runtime (capi_enc.inc) reaches it through the functions picture_host.h declares.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include "../../include/h264mi.h"
#include "picture_host.h"

namespace h264mi {
#define SDEV __device__ __forceinline__

#define H264MI_SCALE_ROWS 16          // output rows per wave
#define H264MI_SCALE_BATCH 8          // source rows whose loads are in flight together

struct ScalePlane { int pw, ph, qw, qh, nstrip, nseg; };  // source, destination samples; waves across / down
struct ScaleLaunch {
    const uint8_t *src;
    uint8_t *dst;
    size_t sfb, dfb;         // frame f: src + f * sfb, dst + f * dfb
    size_t soff[3], doff[3]; // a frame's planes
    int n, nwaves;           // frames; waves per frame = luma waves + 2 * chroma waves
    ScalePlane pl[2];        // luma, chroma
};

// the horizontal sums of one output column on H264MI_SCALE_BATCH source rows (row r at row + r * stride[r]):
// wf p[i0] + qw (p[i0+1] + .. + p[i1-1]) + wl p[i1] each (wl = 0 when i1 == i0), from byte loads. The rows' loads of
// one tap are independent of each other and issued together.
SDEV void scale_hsum_bytes(uint32_t *h, const uint8_t *const *row, int i0, int i1, uint32_t wf, uint32_t wl, uint32_t qw) {
    uint32_t mid[H264MI_SCALE_BATCH];
#pragma unroll
    for (int r = 0; r < H264MI_SCALE_BATCH; r++) mid[r] = 0;
    for (int i = i0 + 1; i < i1; i++) {
#pragma unroll
        for (int r = 0; r < H264MI_SCALE_BATCH; r++) mid[r] += row[r][i];
    }
#pragma unroll
    for (int r = 0; r < H264MI_SCALE_BATCH; r++) h[r] = wf * row[r][i0] + qw * mid[r] + wl * row[r][i1];
}
// the same from the aligned dwords i0 / 4 .. i1 / 4 of rows that start at a multiple of 4: the taps between the
// first and the last are summed by v_sad_u8 under a byte mask, which the rows share
SDEV void scale_hsum_dwords(uint32_t *h, const uint8_t *const *row, int i0, int i1, uint32_t wf, uint32_t wl, uint32_t qw) {
    const int d0 = i0 >> 2, d1 = i1 >> 2;
    uint32_t mid[H264MI_SCALE_BATCH], first[H264MI_SCALE_BATCH], last[H264MI_SCALE_BATCH];
#pragma unroll
    for (int r = 0; r < H264MI_SCALE_BATCH; r++) mid[r] = first[r] = last[r] = 0;
    for (int d = d0; d <= d1; d++) {
        uint32_t v[H264MI_SCALE_BATCH];
#pragma unroll
        for (int r = 0; r < H264MI_SCALE_BATCH; r++) v[r] = ((const uint32_t *)row[r])[d];
        const int lo = max(i0 + 1 - 4 * d, 0), hi = min(i1 - 1 - 4 * d, 3);  // the dword's bytes between the end taps
        const uint32_t m = lo <= hi ? (0xffffffffu >> (8 * (3 - hi))) & (0xffffffffu << (8 * lo)) : 0u;
#pragma unroll
        for (int r = 0; r < H264MI_SCALE_BATCH; r++) {
            mid[r] = __builtin_amdgcn_sad_u8(v[r] & m, 0u, mid[r]);
            if (d == d0) first[r] = (v[r] >> (8 * (i0 & 3))) & 255u;
            if (d == d1) last[r] = (v[r] >> (8 * (i1 & 3))) & 255u;
        }
    }
#pragma unroll
    for (int r = 0; r < H264MI_SCALE_BATCH; r++) h[r] = wf * first[r] + qw * mid[r] + wl * last[r];
}

__global__ __launch_bounds__(256) void scale_kernel(ScaleLaunch a) {
    const int lane = threadIdx.x & 63;
    const int lw = a.pl[0].nstrip * a.pl[0].nseg, cwv = a.pl[1].nstrip * a.pl[1].nseg;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // scalar: what follows from it is per wave
    const long long items = (long long)a.n * a.nwaves;
    for (long long it = (long long)blockIdx.x * 4 + wave; it < items; it += (long long)gridDim.x * 4) {
        const long long f = it / a.nwaves;
        int k = (int)(it - f * a.nwaves);  // the wave's index within a frame
        int p = 0;
        if (k >= lw) { k -= lw; p = 1; if (k >= cwv) { k -= cwv; p = 2; } }
        const ScalePlane g = a.pl[p != 0];
        const uint8_t *S = a.src + (size_t)f * a.sfb + a.soff[p];
        uint8_t *D = a.dst + (size_t)f * a.dfb + a.doff[p];
        const bool wide = ((((uintptr_t)S) | (uintptr_t)g.pw) & 3) == 0;
        const int strip = k % g.nstrip, seg = k / g.nstrip;
        const int ox = strip * 64 + lane;
        const bool act = ox < g.qw;
        // the lane's taps: columns i0..i1, weights wf, qw, .., qw, wl
        int i0 = 0, i1 = 0;
        uint32_t wf = 0, wl = 0;
        if (act) {
            const int lo = ox * g.pw, hi = lo + g.pw;  // the output column in units of 1 / (pw qw)
            i0 = lo / g.qw;
            i1 = (hi + g.qw - 1) / g.qw - 1;
            wf = (uint32_t)(min((i0 + 1) * g.qw, hi) - lo);
            wl = i1 > i0 ? (uint32_t)(hi - i1 * g.qw) : 0u;
        }
        const uint32_t area = (uint32_t)g.pw * (uint32_t)g.ph, half = area >> 1;
        const int oy0 = seg * H264MI_SCALE_ROWS, oy1 = min(oy0 + H264MI_SCALE_ROWS, g.qh);
        const int y0 = (oy0 * g.ph) / g.qh, y1 = (oy1 * g.ph + g.qh - 1) / g.qh - 1;  // source rows y0..y1
        int oy = oy0;
        uint32_t acc = 0;
        for (int yb0 = y0; yb0 <= y1; yb0 += H264MI_SCALE_BATCH) {  // a batch of source rows: its loads, then the rows in order
            uint32_t hs[H264MI_SCALE_BATCH];
#pragma unroll
            for (int r = 0; r < H264MI_SCALE_BATCH; r++) hs[r] = 0;
            if (act) {
                const uint8_t *row[H264MI_SCALE_BATCH];  // rows beyond y1 read row y1 again and are not used
#pragma unroll
                for (int r = 0; r < H264MI_SCALE_BATCH; r++) row[r] = S + (size_t)min(yb0 + r, y1) * g.pw;
                if (wide) scale_hsum_dwords(hs, row, i0, i1, wf, wl, (uint32_t)g.qw);
                else scale_hsum_bytes(hs, row, i0, i1, wf, wl, (uint32_t)g.qw);
            }
#pragma unroll
            for (int r = 0; r < H264MI_SCALE_BATCH; r++) {
            const int y = yb0 + r;
            if (y > y1) break;
            const uint32_t h = hs[r];
            const int top = oy * g.ph, bot = top + g.ph, ya = y * g.qh, yb = ya + g.qh;  // the same in every lane
            acc += (uint32_t)(min(yb, bot) - max(ya, top)) * h;
            if (yb >= bot) {  // output row oy is complete
                const uint32_t v = (acc + half) / area;
                uint8_t *o = D + (size_t)oy * g.qw + strip * 64;  // the strip's first sample of the row
                if (((uintptr_t)o & 3) == 0) {
                    uint32_t q = v | (__shfl_down(v, 1) << 8);
                    q |= __shfl_down(q, 2) << 16;  // lanes 4j: the bytes of lanes 4j .. 4j + 3
                    if (act) {
                        const int base = ox & ~3;
                        if (base + 3 < g.qw) { if ((lane & 3) == 0) *(uint32_t *)(o + lane) = q; }
                        else o[lane] = (uint8_t)v;
                    }
                } else if (act) {
                    o[lane] = (uint8_t)v;
                }
                oy++;
                acc = (uint32_t)(yb - bot) * h;  // the rest of a straddling row opens the next one
            }
            }
        }
    }
}

// arguments of a scale call: even sizes, 2 <= dw <= sw <= 4096, 2 <= dh <= sh <= 4096
bool scale_args_ok(int dw, int dh, int sw, int sh, int n) { return n > 0 && sides_ok(dw, dh, sw, sh) && dw <= sw && dh <= sh; }
static ScalePlane scale_plane(int pw, int ph, int qw, int qh) {
    return ScalePlane{pw, ph, qw, qh, (qw + 63) / 64, (qh + H264MI_SCALE_ROWS - 1) / H264MI_SCALE_ROWS};
}
// n tight sw x sh I420 frames at src to n tight dw x dh frames at dst; arguments as scale_args_ok accepts them
int launch_scale_i420(uint8_t *dst, int dw, int dh, const uint8_t *src, int sw, int sh, int n, hipStream_t s) {
    const size_t sy = (size_t)sw * sh, sc = (size_t)(sw / 2) * (sh / 2), dy = (size_t)dw * dh, dc = (size_t)(dw / 2) * (dh / 2);
    ScaleLaunch a{};
    a.src = src; a.dst = dst; a.sfb = sy + 2 * sc; a.dfb = dy + 2 * dc;
    a.soff[0] = 0; a.soff[1] = sy; a.soff[2] = sy + sc;
    a.doff[0] = 0; a.doff[1] = dy; a.doff[2] = dy + dc;
    a.n = n;
    a.pl[0] = scale_plane(sw, sh, dw, dh);
    a.pl[1] = scale_plane(sw / 2, sh / 2, dw / 2, dh / 2);
    a.nwaves = a.pl[0].nstrip * a.pl[0].nseg + 2 * a.pl[1].nstrip * a.pl[1].nseg;
    (void)hipGetLastError();
    hipLaunchKernelGGL(scale_kernel, dim3(launch_blocks((long long)n * a.nwaves)), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace h264mi
