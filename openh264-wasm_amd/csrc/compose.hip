// compose.hip -- several I420 pictures into one on the device (gfx950), as include/h264mi.h defines it
// (h264mi_i420_compose_dev, h264mi_i420_fill_dev, h264mi_mosaic_cells). DESIGN.md §5.4.
//   compose_kernel : up to H264MI_COMPOSE_CELLS cells per launch -- the standalone call, or sources composed into an
//                    encoder's input area (h264mi_enc_encode_composed)
//   fill_kernel    : n tight frames set to one colour
// A cell takes a crop of one source frame to a rectangle of one canvas. Per plane that is §5.3's area average with
// pw x ph = the crop's size in the plane and qw x qh = the rectangle's (scale.hip's header has the formula): exact
// unsigned 32-bit integers for pw, ph <= 4096, the same bytes whatever the order of evaluation.
// The walk is scale_kernel's, picture_dev.h's area_average: a wave owns a strip of 64 output columns and a segment of PIC_AREA_ROWS output rows
// of one plane of one cell and walks the overlapping source rows downward, PIC_AREA_BATCH rows at a time, a lane
// per output column. What differs:
//  * geometry is per cell. The launch's arguments hold the cells and a prefix table of waves per cell; a wave finds its
//    cell by a binary search of that table (all of it scalar), then plane, strip and segment as the scaler does.
//  * rows are a pitch apart that is not the plane's width: source rows the source plane's width, destination rows the
//    canvas plane's. A lane's taps are columns of the source plane row: the crop's first column added to the taps within
//    the crop.
//  * a source plane is read as dwords when its base address and its pitch are multiples of 4, whatever the crop's first
//    column: the aligned dwords that hold the taps lie in the same plane row (the pitch is a multiple of 4 and every tap
//    is below it), the samples of such a dword that are not taps are masked out or shifted away. Otherwise bytes.
//  * an output row segment is stored as dwords when its first address is a multiple of 4 -- tested per row, since with a
//    canvas pitch that is no multiple of 4 it changes from row to row -- and then only the groups of four samples that
//    lie inside the rectangle; everything else as bytes. Nothing is written outside the rectangle, nothing is read
//    outside the source frame.
//
// A translation unit and a code object of its own, as quality.hip and scale.hip are. The host runtime (capi_enc.inc) reaches it through the functions picture_host.h declares;
// the checks of a cell list and the cell table of a launch are there too.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include "../../include/h264mi.h"
#include "picture_host.h"
#include "picture_dev.h"

namespace h264mi {
#define H264MI_COMPOSE_CELLS 64         // cells per launch: the argument block is 1.9 KB

typedef PictureCell ComposeCell;  // a cell as the kernel reads it, 24 bytes (picture_host.h)
struct ComposeLaunch {
    const uint8_t *src;
    uint8_t *dst;
    size_t sfb, dfb;                           // source frame f: src + f * sfb; canvas c: dst + c * dfb
    int src_w, src_h, cw, ch;
    int ncells;
    int first[H264MI_COMPOSE_CELLS + 1];       // cell k's waves are first[k] .. first[k + 1] - 1
    ComposeCell cell[H264MI_COMPOSE_CELLS];
};
static_assert(sizeof(ComposeLaunch) < 2048, "the argument block stays well below 4 KB");

__global__ __launch_bounds__(256) void compose_kernel(ComposeLaunch a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // scalar: what follows from it is per wave
    const int items = a.first[a.ncells];
    for (int it = (int)blockIdx.x * 4 + wave; it < items; it += (int)gridDim.x * 4) {
        int lo_c = 0, hi_c = a.ncells;  // first[lo_c] <= it < first[hi_c]
        while (hi_c - lo_c > 1) {
            const int mid_c = (lo_c + hi_c) >> 1;
            if (a.first[mid_c] <= it) lo_c = mid_c; else hi_c = mid_c;
        }
        const ComposeCell c = a.cell[lo_c];
        int k = it - a.first[lo_c];  // the wave's index within the cell
        const int lw = area_nstrip(c.dw) * area_nseg(c.dh), cwv = area_nstrip(c.dw >> 1) * area_nseg(c.dh >> 1);
        int p = 0;
        if (k >= lw) { k -= lw; p = 1; if (k >= cwv) { k -= cwv; p = 2; } }
        const int sh1 = p != 0;  // chroma: every size and origin halved
        const int pw = c.sw >> sh1, ph = c.sh >> sh1, qw = c.dw >> sh1, qh = c.dh >> sh1;
        const int spitch = a.src_w >> sh1, dpitch = a.cw >> sh1;
        const size_t sy_b = (size_t)a.src_w * a.src_h, sc_b = (size_t)(a.src_w >> 1) * (a.src_h >> 1);
        const size_t dy_b = (size_t)a.cw * a.ch, dc_b = (size_t)(a.cw >> 1) * (a.ch >> 1);
        // the source plane, and its row that holds the crop's first row; the rectangle's first sample
        const uint8_t *P = a.src + (size_t)c.src * a.sfb + (p == 0 ? 0 : p == 1 ? sy_b : sy_b + sc_b);
        const uint8_t *S = P + (size_t)(c.sy >> sh1) * spitch;
        uint8_t *D = a.dst + (size_t)c.canvas * a.dfb + (p == 0 ? 0 : p == 1 ? dy_b : dy_b + dc_b) + (size_t)(c.dy >> sh1) * dpitch +
                     (c.dx >> sh1);
        const int x0 = c.sx >> sh1;
        const bool wide = ((((uintptr_t)P) | (uintptr_t)spitch) & 3) == 0;
        const int nstrip = area_nstrip(qw);
        area_average(D, dpitch, S, spitch, wide, x0, pw, ph, qw, qh, k % nstrip, k / nstrip, lane);
    }
}

// n tight w x h frames at dst set to (y, cb, cr). blockIdx.y is the frame; a thread owns aligned 16-byte pieces of the
// frame's address range: one inside a plane and inside the frame is one store, any other goes byte by byte, each byte
// tested against the frame's range (the piece's other bytes are a neighbouring frame's, or nobody's).
struct FillLaunch {
    uint8_t *dst;
    size_t fb, yb, cb;  // bytes of a frame, of its luma plane, of one chroma plane
    uint32_t v[3];      // the three values, each in all four bytes
};
__global__ __launch_bounds__(256) void fill_kernel(FillLaunch a) {
    const uintptr_t lo = (uintptr_t)a.dst + (size_t)blockIdx.y * a.fb, hi = lo + a.fb;  // the frame's bytes
    const uintptr_t first = lo & ~(uintptr_t)15;
    const size_t pieces = (hi - first + 15) >> 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < pieces; i += (size_t)gridDim.x * blockDim.x) {
        const uintptr_t p = first + (i << 4);
        if (p >= lo && p + 16 <= hi) {
            const size_t off = p - lo;  // plane of the piece's first and last byte
            const int p0 = off < a.yb ? 0 : off < a.yb + a.cb ? 1 : 2, p1 = off + 15 < a.yb ? 0 : off + 15 < a.yb + a.cb ? 1 : 2;
            if (p0 == p1) {
                const uint32_t v = a.v[p0];
                *(uint4 *)p = make_uint4(v, v, v, v);
                continue;
            }
        }
        for (int b = 0; b < 16; b++) {
            const uintptr_t q = p + b;
            if (q < lo || q >= hi) continue;
            const size_t off = q - lo;
            *(uint8_t *)q = (uint8_t)a.v[off < a.yb ? 0 : off < a.yb + a.cb ? 1 : 2];
        }
    }
}

// arguments of a fill call
bool fill_args_ok(int w, int h, int n, int y, int cb, int cr) {
    return n > 0 && canvas_ok(w, h) && y >= 0 && y <= 255 && cb >= 0 && cb <= 255 && cr >= 0 && cr <= 255;
}
int launch_fill_i420(uint8_t *dst, int w, int h, int n, int y, int cb, int cr, hipStream_t s) {
    FillLaunch a{};
    a.dst = dst; a.fb = i420_bytes(w, h); a.yb = (size_t)w * h; a.cb = (size_t)(w / 2) * (h / 2);
    a.v[0] = 0x01010101u * (uint32_t)y; a.v[1] = 0x01010101u * (uint32_t)cb; a.v[2] = 0x01010101u * (uint32_t)cr;
    const size_t blocks = (a.fb / 16 + 2 + 255) / 256;
    const unsigned gx = (unsigned)std::min(blocks, (size_t)std::max(1, PIC_MAX_BLOCKS / n));
    (void)hipGetLastError();
    for (int f0 = 0; f0 < n; f0 += 65535) {  // gridDim.y is 16 bits
        FillLaunch b = a;
        b.dst = dst + (size_t)f0 * a.fb;
        hipLaunchKernelGGL(fill_kernel, dim3(gx, (unsigned)std::min(n - f0, 65535)), dim3(256), 0, s, b);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

static int compose_cell_waves(int dw, int dh) {
    return area_nstrip(dw) * area_nseg(dh) + 2 * area_nstrip(dw / 2) * area_nseg(dh / 2);
}
// cells (as cells_ok accepts them without enlarging) into the canvases at dst, H264MI_COMPOSE_CELLS to a launch
int launch_compose_i420(uint8_t *dst, int cw, int ch, const uint8_t *src, int src_w, int src_h, const h264mi_cell *cells, int ncells,
                        hipStream_t s) {
    ComposeLaunch a{};
    a.src = src; a.dst = dst; a.sfb = i420_bytes(src_w, src_h); a.dfb = i420_bytes(cw, ch);
    a.src_w = src_w; a.src_h = src_h; a.cw = cw; a.ch = ch;
    (void)hipGetLastError();
    for (int k0 = 0; k0 < ncells; k0 += H264MI_COMPOSE_CELLS) {
        a.ncells = fill_cell_table(a.cell, a.first, cells + k0, std::min(ncells - k0, H264MI_COMPOSE_CELLS), compose_cell_waves);
        hipLaunchKernelGGL(compose_kernel, dim3(launch_blocks(a.first[a.ncells])), dim3(256), 0, s, a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// the gallery layout of include/h264mi.h (h264mi_mosaic_cells): host only, integers, floor divisions
int mosaic_cells(h264mi_cell *out, int cap, int n, int src_w, int src_h, int cw, int ch) {
    if (!layout_args_ok(out, cap, n, src_w, src_h, cw, ch)) return -1;
    int cols = 1;
    while (cols * cols < n) cols++;
    const int rows = (n + cols - 1) / cols;
    for (int k = 0; k < n; k++) {
        const int col = k % cols, row = k / cols;
        const int X0 = 2 * (col * cw / (2 * cols)), X1 = 2 * ((col + 1) * cw / (2 * cols));
        const int Y0 = 2 * (row * ch / (2 * rows)), Y1 = 2 * ((row + 1) * ch / (2 * rows));
        if (!fit_centred(out + k, k, src_w, src_h, X0, X1, Y0, Y1, false)) return -1;
    }
    return n;
}
}  // namespace h264mi
