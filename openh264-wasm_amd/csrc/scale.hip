// scale.hip -- area-average downscaling of tight I420 frames on the device (gfx950), as include/h264mi.h
// (h264mi_i420_scale_dev) defines it. DESIGN.md §5.3.
//   scale_kernel : n frames of one geometry pair per launch -- the standalone call, or an encoder's source frames
//                  scaled into its input area (h264mi_enc_encode_scaled)
// Every plane is scaled on its own (Y sw x sh -> dw x dh; Cb, Cr sw/2 x sh/2 -> dw/2 x dh/2). For a plane of
// pw x ph samples scaled to qw x qh, source column i weighs max(0, min((i+1) qw, (ox+1) pw) - max(i qw, ox pw)) in
// output column ox, rows likewise with ph, qh, and out = (sum wy wx p + (pw ph >> 1)) / (pw ph). The sum is
// separable, every partial is an integer, and with pw, ph <= 4096 the numerator stays below 2^32: unsigned 32-bit
// accumulation is exact and the result does not depend on the order of evaluation.
// A wave owns a strip of 64 output columns and a segment of PIC_AREA_ROWS output rows of one plane of one
// frame and walks the overlapping source rows downward: per source row a lane forms the horizontal sum of its
// output column (its taps i0..i1 and their weights are the same on every row: the first and last tap weigh wf and
// wl, every tap between them qw), adds wy times it to the accumulator of the current output row and, when the
// source row straddles two output rows, starts the next row's accumulator with the rest. An output row is stored
// once its last source row has gone by, so inside a strip segment a source sample is loaded once (adjacent strips
// share at most one column, adjacent segments one row). The taps are a loop: 1 to ceil(pw / qw) + 1 of them.
// The source rows are taken PIC_AREA_BATCH at a time: the horizontal sums of a batch are formed together, so
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
// This file owns the formula, the frame-wise launch and its checks; the walk of a strip segment (area_average: taps,
// horizontal sums, batch loop, dword store) is picture_dev.h's, which compose.hip uses too.
// A translation unit and a code object of its own, as quality.hip is. The host runtime (capi_enc.inc) reaches it through the functions picture_host.h declares.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include "../../include/h264mi.h"
#include "picture_host.h"
#include "picture_dev.h"

namespace h264mi {
struct ScalePlane { int pw, ph, qw, qh, nstrip, nseg; };  // source, destination samples; waves across / down
struct ScaleLaunch {
    const uint8_t *src;
    uint8_t *dst;
    size_t sfb, dfb;         // frame f: src + f * sfb, dst + f * dfb
    size_t soff[3], doff[3]; // a frame's planes
    int n, nwaves;           // frames; waves per frame = luma waves + 2 * chroma waves
    ScalePlane pl[2];        // luma, chroma
};

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
        area_average(D, g.qw, S, g.pw, wide, 0, g.pw, g.ph, g.qw, g.qh, strip, seg, lane);
    }
}

// arguments of a scale call: even sizes, 2 <= dw <= sw <= 4096, 2 <= dh <= sh <= 4096
bool scale_args_ok(int dw, int dh, int sw, int sh, int n) { return n > 0 && sides_ok(dw, dh, sw, sh) && dw <= sw && dh <= sh; }
static ScalePlane scale_plane(int pw, int ph, int qw, int qh) {
    return ScalePlane{pw, ph, qw, qh, area_nstrip(qw), area_nseg(qh)};
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
