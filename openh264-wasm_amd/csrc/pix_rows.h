// pix_rows.h -- the row-pair frame that pixfmt.hip and pixdeep.hip share: the v_perm_b32
// selectors, the alignment test, the row move and the byte average, a frame with both sides resolved, the launch
// structs, the batch kernel and the decoder read-out kernel, and their host launchers. Kernels and launchers are
// templates over the unit's row-pair function (PixRowPair), which is inlined: each unit instantiates its own in its
// own code object and keeps only its formats' row functions.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include "../../include/h264mi.h"
#include "h264mi_types.h"
#include "picture_host.h"
#include "picture_dev.h"

namespace h264mi {
#define PIX_STRIP 4   // row pairs per block, one per wave

// v_perm_b32 selectors: bytes 0..3 name the second operand's bytes, 4..7 the first's, 0x0c is the constant 0
#define PIX_SEL_ZIP_LO 0x05010400u   // (hi, lo) -> lo.0 hi.0 lo.1 hi.1
#define PIX_SEL_ZIP_HI 0x07030602u   // (hi, lo) -> lo.2 hi.2 lo.3 hi.3
#define PIX_SEL_EVEN 0x06040200u     // (hi, lo) -> lo.0 lo.2 hi.0 hi.2
#define PIX_SEL_ODD 0x07050301u      // (hi, lo) -> lo.1 lo.3 hi.1 hi.3
#define PIX_SEL_WIDE_LO 0x0c010c00u  // (-, x) -> x.0 0 x.1 0
#define PIX_SEL_WIDE_HI 0x0c030c02u  // (-, x) -> x.2 0 x.3 0

// one frame, both sides resolved: the layout side's planes p[] with pitches pp[], the I420 side's planes with pitches;
// depth: the rule of h264mi_pixopt, which only the 10-bit formats read
struct PixFrame {
    uint8_t *p[3];
    int pp[3];
    uint8_t *y, *u, *v;
    int ys, cs;
    int w, h, pix, depth;
};

PICDEV bool pix_al(const void *a, const void *b, unsigned mask) { return ((((uintptr_t)a) | ((uintptr_t)b)) & mask) == 0; }

// rows (1 or 2) rows of nb bytes from s (pitch sp) to d (pitch dp)
PICDEV void pix_move_rows(uint8_t *d, int dp, const uint8_t *s, int sp, int nb, int rows, int lane) {
    const bool wide = pix_al(d, s, 15) && (rows == 1 || pix_al(d + dp, s + sp, 15));
    for (int x = 16 * lane; x < nb; x += 16 * 64) {
        if (wide && x + 16 <= nb) {
            const uint4 a = *(const uint4 *)(s + x);
            if (rows == 2) {
                const uint4 b = *(const uint4 *)(s + sp + x);
                *(uint4 *)(d + dp + x) = b;
            }
            *(uint4 *)(d + x) = a;
        } else {
            for (int r = 0; r < rows; r++)
                for (int j = 0; j < 16 && x + j < nb; j++) d[(size_t)r * dp + x + j] = s[(size_t)r * sp + x + j];
        }
    }
}

// (x + y + 1) >> 1 of the four bytes of x and y
PICDEV uint32_t pix_avg4(uint32_t x, uint32_t y) {
    const uint32_t lo = __builtin_amdgcn_perm(0u, x, PIX_SEL_WIDE_LO) + __builtin_amdgcn_perm(0u, y, PIX_SEL_WIDE_LO) + 0x00010001u;
    const uint32_t hi = __builtin_amdgcn_perm(0u, x, PIX_SEL_WIDE_HI) + __builtin_amdgcn_perm(0u, y, PIX_SEL_WIDE_HI) + 0x00010001u;
    return __builtin_amdgcn_perm(hi >> 1, lo >> 1, PIX_SEL_EVEN);  // the low byte of each 16-bit field: sums are below 512
}

// row pair r (luma rows 2r, 2r + 1, I420 chroma row r) of a frame, one wave: from the layout side to the I420 side or back
typedef void (*PixRowPair)(const PixFrame &f, int r, int lane);

struct PixLaunch {
    uint8_t *pk;          // the layout side: frame f at pk + f * pk_fs, plane p at + off[p], pitch[p]
    uint8_t *i420;        // the I420 side, tight: frame f at i420 + f * fb
    int64_t pk_fs, off[3];
    size_t fb;
    int pitch[3];
    int pix, w, h, n, nstrip, depth;
};

// n frames between a layout and tight I420, whichever way ROWS goes
template <PixRowPair ROWS>
__global__ __launch_bounds__(256) void pix_rows_kernel(PixLaunch a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long items = (long long)a.n * a.nstrip;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long fi = it / a.nstrip;
        const int r = (int)(it - fi * a.nstrip) * PIX_STRIP + wv;
        if (r >= a.h / 2) continue;
        PixFrame f;
        uint8_t *pk = a.pk + fi * a.pk_fs, *fr = a.i420 + (size_t)fi * a.fb;
        for (int p = 0; p < 3; p++) { f.p[p] = pk + a.off[p]; f.pp[p] = a.pitch[p]; }
        f.y = fr; f.u = fr + (size_t)a.w * a.h; f.v = f.u + (size_t)(a.w / 2) * (a.h / 2);
        f.ys = a.w; f.cs = a.w / 2;
        f.w = a.w; f.h = a.h; f.pix = a.pix; f.depth = a.depth;
        ROWS(f, r, lane);
    }
}

// Read-out of a batched decode call into a layout (after dec_end_kernel of frame f): what dec_output_kernel does for
// tight I420 -- got, and the picture pic[outpar] cropped by its SPS, read where it lies (coded strides, crop origin) --
// written in layout lay to in[s].out. lay was checked for w x h; a picture of another cropped size is not written. A
// frame whose base I.out is no multiple of the format's unit is reported in got but not written (the host cannot see it)
struct DecPixLaunch { int S, cw, ch, w, h, nstrip, unit; const DecDesc *desc; const DecInput *in; h264mi_pix_layout lay; };
template <PixRowPair ROWS>
__global__ __launch_bounds__(256) void dec_output_rows_kernel(DecPixLaunch a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int items = a.S * a.nstrip;
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        const int s = it / a.nstrip, k = it - s * a.nstrip;
        const DecState *st = a.desc[s].st;
        const DecInput &I = a.in[s];
        const int ok = st->got_pic && !st->err;
        if (I.got && k == 0 && threadIdx.x == 0) *I.got = ok;
        if (!ok || !I.out || (((uintptr_t)I.out) & (uintptr_t)(a.unit - 1))) continue;
        const int c0 = st->ps.crop[0], c1 = st->ps.crop[1], c2 = st->ps.crop[2], c3 = st->ps.crop[3];
        const int W = a.cw - 2 * (c0 + c1), H = a.ch - 2 * (c2 + c3), x0 = 2 * c0, y0 = 2 * c2;
        const int r = k * PIX_STRIP + wv;
        if (W != a.w || H != a.h || r >= H / 2) continue;
        uint8_t *const *pic = a.desc[s].pic[st->outpar & 1];
        PixFrame f;
        for (int p = 0; p < 3; p++) { f.p[p] = I.out + a.lay.offset[p]; f.pp[p] = a.lay.pitch[p]; }
        f.ys = a.cw; f.cs = a.cw / 2;
        f.y = pic[0] + (size_t)y0 * f.ys + x0;
        f.u = pic[1] + (size_t)(y0 / 2) * f.cs + x0 / 2;
        f.v = pic[2] + (size_t)(y0 / 2) * f.cs + x0 / 2;
        f.w = W; f.h = H; f.pix = a.lay.pix; f.depth = 0;
        ROWS(f, r, lane);
    }
}

// ---- host
static inline int pix_nstrip(int h) { return (h / 2 + PIX_STRIP - 1) / PIX_STRIP; }
// n frames between layout L at pk and tight I420 at i420; arguments as pix_args_ok accepts them. The side that is only
// read comes in without its const
template <PixRowPair ROWS>
int launch_pix_rows(const void *pk, const h264mi_pix_layout &L, const void *i420, int depth, int w, int h, int n, hipStream_t s) {
    PixLaunch a{};
    a.pk = (uint8_t *)pk; a.i420 = (uint8_t *)i420; a.pk_fs = L.frame_stride; a.fb = i420_bytes(w, h);
    for (int p = 0; p < 3; p++) { a.off[p] = L.offset[p]; a.pitch[p] = L.pitch[p]; }
    a.pix = L.pix; a.w = w; a.h = h; a.n = n; a.nstrip = pix_nstrip(h); a.depth = depth;  // at most 1024 strips a frame
    const unsigned blocks = (unsigned)std::min((long long)n * a.nstrip, (long long)PIC_MAX_BLOCKS);
    (void)hipGetLastError();
    hipLaunchKernelGGL(pix_rows_kernel<ROWS>, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// frame f's S entries of desc / in, as DecOutLaunch holds them; L good for w x h (h264mi_dec_set_output_layout)
template <PixRowPair ROWS>
int launch_dec_output_rows(int S, int cw, int ch, int w, int h, const DecDesc *desc, const DecInput *in, const h264mi_pix_layout &L,
                           hipStream_t s) {
    DecPixLaunch a{S, cw, ch, w, h, pix_nstrip(h), pix_unit(L.pix), desc, in, L};
    const unsigned blocks = (unsigned)std::min(S * a.nstrip, PIC_MAX_BLOCKS);  // S <= 256 streams of <= 1024 strips
    (void)hipGetLastError();
    hipLaunchKernelGGL(dec_output_rows_kernel<ROWS>, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace h264mi
