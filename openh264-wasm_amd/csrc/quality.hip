// quality.hip -- per-frame distortion of picture pairs on the device (gfx950): the sum of squared differences and
// the fixed-point SSIM sum of every plane, as include/h264mi.h (h264mi_quality) defines them. DESIGN.md §5.2.
//   quality_kernel : n pairs of pictures (a, b) per launch -- the standalone call's tight I420 frames, or an
//                    encoder's source frames against the display area of that step's deblocked pictures
// A plane of pw x ph samples is cut into 4x4 blocks (bw = pw / 4 by bh = ph / 4 whole blocks); an SSIM window
// (8x8 at stride 4) is a 2x2 group of blocks, so there are (bw - 1)(bh - 1) of them. A wave owns a strip of 64
// block columns and H264MI_QUAL_ROWS block rows of one plane of one pair and walks it downward: a lane reads
// its block as one dword per row from each picture (a wave reads 256 contiguous bytes of a row), takes
// sum a, sum b (v_sad_u8 against 0) and sum ab, sum a^2 + b^2 (v_dot4_u32_u8), adds its right neighbour's sums
// (strips overlap by one column: lane 63 only lends its block) and keeps the previous block row's pair sums in
// registers, so a sample is loaded once inside a strip segment (segments re-read one block row, strips one
// block column: 8 % at 1080p). A window's value is integer arithmetic up to one double division and one
// rounding to int64 (both single correctly rounded IEEE-754 operations); every partial is an integer, so the
// totals do not depend on the order of addition: lanes add in registers, waves by shuffles, and one 64-bit
// integer atomic add per wave and statistic lands in the record the host zeroed on the same stream.
// Squared errors: a lane meets at most 16 * H264MI_QUAL_ROWS + a few tail samples (32 bits hold 66 051); every
// sum across lanes is 64 bits wide. Samples right of / below the last whole block (pw % 4, ph % 4) count in
// the SSE only: the plane's waves share them as a lane-strided byte loop.
// A plane whose rows cannot be read as dwords (a base address or a stride that is no multiple of 4: w % 8 != 0
// chroma, a buffer at an odd address) takes byte loads assembled into the same dwords -- the same sums. The test
// is per plane and pair, from the plane's own pointers, as color.inc's is per frame. (hipcc for gfx950 today merges
// the four byte loads back into one unaligned dword load, which global memory accepts; the source does not rely on it.)
// No access leaves the pw x ph area of either picture.
//
// A translation unit and a code object of its own: the library's other kernels stay in theirs, byte for byte what
// they were, and an encoder that never turns the records on runs exactly the device code it ran before. The host
// runtime (runtime_enc.inc, capi_enc.inc) reaches it through the three functions at the end, which picture_host.h declares.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include "../../include/h264mi.h"
#include "h264mi_types.h"
#include "picture_host.h"
#include "picture_dev.h"

namespace h264mi {
#define H264MI_QUAL_ROWS 16     // block rows (of windows) per wave
#define H264MI_QUAL_COLS 63     // block columns (of windows) per wave: 64 lanes, the last one lends its block
#define H264MI_QUAL_MAX_PAIRS_Y 32768

struct QualPlane { int pw, ph, bw, bh, nstrip, nseg; };  // samples, whole 4x4 blocks, waves across / down
struct QualLaunch {
    const uint8_t *a, *b;    // pair f: pictures at a + f * afs and b + f * bfs (b: unless desc)
    size_t afs, bfs;
    size_t aoff[3], boff[3]; // a picture's planes
    int sa[2], sb[2];        // row strides, luma / chroma
    const EncDesc *desc;     // encoder: pair f's b planes are desc[f].dbk[], and a pair whose stream published
                             // no NAL bytes (desc[f].st->nal_bytes == 0) is left as the host zeroed it
    h264mi_quality *out;
    int n, nwaves;           // pairs; waves per pair = luma waves + 2 * chroma waves
    QualPlane pl[2];         // luma, chroma
};

PICDEV uint32_t qual_ld4(const uint8_t *p, bool narrow) {
    if (narrow) return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    return *(const uint32_t *)p;
}
PICDEV uint64_t qual_wave_sum(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;  // lane 0
}

__global__ __launch_bounds__(256) void quality_kernel(QualLaunch q) {
    const int lane = threadIdx.x & 63;
    int k = blockIdx.x * 4 + (threadIdx.x >> 6);  // the wave's index within a pair
    if (k >= q.nwaves) return;
    const int lw = q.pl[0].nstrip * q.pl[0].nseg, cwv = q.pl[1].nstrip * q.pl[1].nseg;
    int p = 0;
    if (k >= lw) { k -= lw; p = 1; if (k >= cwv) { k -= cwv; p = 2; } }
    const QualPlane g = q.pl[p != 0];
    const int per = p ? cwv : lw;
    const int sa = q.sa[p != 0], sb = q.sb[p != 0];
    const int strip = k % g.nstrip, seg = k / g.nstrip;
    const int col = strip * H264MI_QUAL_COLS + lane;
    const bool act = col < g.bw;                                        // the lane has a block column
    const bool wcol = lane < H264MI_QUAL_COLS && col + 1 < g.bw;       // and a window column
    const int r0 = seg * H264MI_QUAL_ROWS, r1 = min(r0 + H264MI_QUAL_ROWS, g.bh - 1);  // block rows read: r0..r1
    const int rt = g.pw - 4 * g.bw, bt = g.ph - 4 * g.bh;               // columns / rows beyond the whole blocks
    const int ntail = rt * g.ph + 4 * g.bw * bt;
    for (int f = blockIdx.y; f < q.n; f += gridDim.y) {
        const uint8_t *A = q.a + (size_t)f * q.afs + q.aoff[p], *B;
        if (q.desc) {
            if (q.desc[f].st->nal_bytes <= 0) continue;  // nothing coded: coded 0, all zeros
            B = q.desc[f].dbk[p];
        } else {
            B = q.b + (size_t)f * q.bfs + q.boff[p];
        }
        const bool narrow = ((((uintptr_t)A | (uintptr_t)B) | (uintptr_t)(sa | sb)) & 3) != 0;
        uint32_t sse = 0;
        int64_t fix = 0;
        uint32_t u1 = 0, us = 0, u12 = 0;  // the block row above: sums of the lane's block and its right neighbour's
        for (int r = r0; r <= r1; r++) {
            uint32_t s1 = 0, s2 = 0, ss = 0, s12 = 0;
            if (act) {
                const uint8_t *pa = A + (size_t)(4 * r) * sa + 4 * col, *pb = B + (size_t)(4 * r) * sb + 4 * col;
#pragma unroll
                for (int y = 0; y < 4; y++) {
                    const uint32_t da = qual_ld4(pa + (size_t)y * sa, narrow), db = qual_ld4(pb + (size_t)y * sb, narrow);
                    s1 = __builtin_amdgcn_sad_u8(da, 0u, s1);
                    s2 = __builtin_amdgcn_sad_u8(db, 0u, s2);
                    ss = __builtin_amdgcn_udot4(da, da, ss, false);
                    ss = __builtin_amdgcn_udot4(db, db, ss, false);
                    s12 = __builtin_amdgcn_udot4(da, db, s12, false);
                }
            }
            // the block's squared error, by the wave that owns the block: row r0 + ROWS and lane 63 are the next one's
            if (lane < H264MI_QUAL_COLS && r < r0 + H264MI_QUAL_ROWS) sse += ss - 2 * s12;
            const uint32_t b1 = s1 | (s2 << 16);  // a block's sums are below 4096, a window's below 16384: no carry
            const uint32_t h1 = b1 + __shfl_down(b1, 1), hs = ss + __shfl_down(ss, 1), h12 = s12 + __shfl_down(s12, 1);
            if (wcol && r > r0) {  // the window of block rows r - 1, r and block columns col, col + 1
                const uint32_t w1 = u1 + h1;
                const int64_t S1 = w1 & 0xffffu, S2 = w1 >> 16, SS = us + hs, S12 = u12 + h12;
                const int64_t vars = 64 * SS - S1 * S1 - S2 * S2, covar = 64 * S12 - S1 * S2;
                const int64_t num = (2 * S1 * S2 + 416) * (2 * covar + 235963);
                const int64_t den = (S1 * S1 + S2 * S2 + 416) * (vars + 235963);
                const double v = (double)num / (double)den;
                fix += (int64_t)llrint(v * 4294967296.0);
            }
            u1 = h1; us = hs; u12 = h12;
        }
        for (int e = k * 64 + lane; e < ntail; e += per * 64) {  // samples in no whole block
            int x, y;
            if (e < rt * g.ph) { y = e / rt; x = 4 * g.bw + (e - y * rt); }
            else { const int t = e - rt * g.ph; y = t / (4 * g.bw); x = t - y * (4 * g.bw); y += 4 * g.bh; }
            const int d = (int)A[(size_t)y * sa + x] - (int)B[(size_t)y * sb + x];
            sse += (uint32_t)(d * d);
        }
        const uint64_t tsse = qual_wave_sum((uint64_t)sse), tfix = qual_wave_sum((uint64_t)fix);
        if (lane == 0) {
            h264mi_quality *o = q.out + f;
            if (tsse) atomicAdd((unsigned long long *)&o->sse[p], (unsigned long long)tsse);
            if (tfix) atomicAdd((unsigned long long *)&o->ssim_fix[p], (unsigned long long)tfix);  // two's complement
            if (p == 0 && k == 0) {
                o->windows[0] = (uint32_t)((q.pl[0].bw - 1) * (q.pl[0].bh - 1));
                o->windows[1] = (uint32_t)((q.pl[1].bw - 1) * (q.pl[1].bh - 1));
                o->coded = 1;
            }
        }
    }
}

// arguments of a quality call: even sizes from 16 (a chroma plane holds a window) whose indices fit an int
bool quality_args_ok(int w, int h, int n) {
    return n > 0 && w >= 16 && h >= 16 && !(w & 1) && !(h & 1) && (long long)w * h < (1LL << 30);
}
static QualPlane qual_plane(int pw, int ph) {
    QualPlane g{pw, ph, pw / 4, ph / 4, 0, 0};
    g.nstrip = (g.bw + H264MI_QUAL_COLS - 1) / H264MI_QUAL_COLS;
    g.nseg = (g.bh + H264MI_QUAL_ROWS - 1) / H264MI_QUAL_ROWS;
    return g;
}
// the w x h area of n pairs; q carries the pictures (a, b or desc, strides, plane offsets) and the records, which
// are zeroed here on the same stream
static int launch_quality(QualLaunch q, int w, int h, int n, hipStream_t s) {
    q.n = n;
    q.pl[0] = qual_plane(w, h);
    q.pl[1] = qual_plane(w / 2, h / 2);
    q.nwaves = q.pl[0].nstrip * q.pl[0].nseg + 2 * q.pl[1].nstrip * q.pl[1].nseg;
    (void)hipGetLastError();
    if (hipMemsetAsync(q.out, 0, sizeof(h264mi_quality) * (size_t)n, s) != hipSuccess) return -1;
    hipLaunchKernelGGL(quality_kernel, dim3((unsigned)((q.nwaves + 3) / 4), (unsigned)std::min(n, H264MI_QUAL_MAX_PAIRS_Y)), dim3(256), 0, s, q);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// n pairs of tight I420 frames back to back
int launch_quality_i420(h264mi_quality *d_out, const uint8_t *a, const uint8_t *b, int w, int h, int n, hipStream_t s) {
    const size_t ysz = (size_t)w * h, csz = (size_t)(w / 2) * (h / 2);
    QualLaunch q{};
    q.a = a; q.b = b; q.afs = q.bfs = ysz + 2 * csz;
    q.aoff[0] = q.boff[0] = 0; q.aoff[1] = q.boff[1] = ysz; q.aoff[2] = q.boff[2] = ysz + csz;
    q.sa[0] = q.sb[0] = w; q.sa[1] = q.sb[1] = w / 2;
    q.desc = nullptr; q.out = d_out;
    return launch_quality(q, w, h, n, s);
}
// an encoder's frame step: the S tight w x h source frames (fbytes apart) against the display area of the deblocked
// pictures desc[s].dbk[] (coded width cw); desc[s].st->nal_bytes == 0 leaves record s cleared
int launch_quality_enc(h264mi_quality *d_out, const uint8_t *d_frames, size_t fbytes, int w, int h, int cw, const EncDesc *desc, int S,
                       hipStream_t s) {
    QualLaunch q{};
    q.a = d_frames; q.afs = fbytes;
    q.aoff[0] = 0; q.aoff[1] = (size_t)w * h; q.aoff[2] = q.aoff[1] + (size_t)(w / 2) * (h / 2);
    q.sa[0] = w; q.sa[1] = w / 2; q.sb[0] = cw; q.sb[1] = cw / 2;
    q.desc = desc; q.out = d_out;
    return launch_quality(q, w, h, S, s);
}
}  // namespace h264mi
