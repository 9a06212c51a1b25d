// denoise.hip -- the temporal denoiser of tight I420 frames on the device (gfx950), as include/h264mi.h
// (h264mi_i420_denoise_dev) defines it. DESIGN.md §5.13.
//   denoise_kernel : n frames of one geometry per launch -- the standalone call, or an encoder's input area filtered
//                    against its state (h264mi_enc_set_denoise)
// The filter. C is the current frame, P the previous filtered one, O the output. Luma is cut into 8 x 8 blocks (smaller
// even ones at the right and lower edge); a block's chroma is the bw/2 x bh/2 rectangle at (4bx, 4by) of Cb and of Cr.
//   gate:   sad = sum |C - P| over the block's luma, npix = bw * bh; moving iff 4 sad > motion * npix; then O = C
//   sample: d = C - P, a = |d|; a >= reach: O = C; else k = K (reach - a) / reach, m = (a k + 128) >> 8,
//           O = C - sign(d) m
// k <= 224 < 256 gives m <= a: O lies between P and C, nothing is clamped. The host builds k[a], a = 0..31, for each
// strength with k[a] = 0 from a = reach on (reach <= 32), so the kernel neither divides nor knows reach: a < 32 looks m
// up, any other a has m = 0.
//
// Work split. A block of four waves owns one strip -- 8 luma rows (one row of blocks) x 256 samples (32 blocks) and the
// strip's 4 x 128 samples of Cb and of Cr -- of one frame. The items (frame, strip row, strip) are dealt to the blocks in
// runs of consecutive items; the loop count depends on the block only, so the barrier is uniform.
//   luma:   thread t holds the 8 bytes x = 8 (t & 31) .. + 7 of row t >> 5: the row of one block. 32 consecutive lanes
//           load and store 256 consecutive bytes of a row, a wave two rows.
//   chroma: thread t holds the 4 bytes 4 (t & 31) .. + 3 of row (t >> 5) & 3 of Cb (t < 128) or Cr: again the row of
//           block t & 31. 32 consecutive lanes cover 128 consecutive bytes.
//   gate:   a thread's luma row gives v_sad_u8 per dword; the eight row sums of a block meet in LDS (sad[row][block],
//           one barrier), and every thread reads the eight of block t & 31: 32 lanes, 32 banks.
// THE ALIASING INVARIANT. d_dst and d_dst2 may be exactly d_cur or exactly d_prev. Every read of a block -- the C and P
// samples of its luma, which are also its SAD, and of its chroma -- is a load that is issued in front of the barrier;
// every write of the block comes after it and stores what was computed from those registers. Blocks of different
// items share no byte, so no thread reads what another has written in the same launch.
// Two paths for the same bytes, chosen per plane and frame from the plane's own pointers and row length: luma whose
// four (three) bases and w are multiples of 8 moves as 8-byte words, chroma whose bases and w / 2 are multiples of 4 as
// dwords; any other plane (a buffer at an odd address, a chroma row of 18 bytes) moves as bytes, gathered into the same
// registers. An aligned word of a row whose length is a multiple of the word never leaves the row, the byte path stops
// at the row's end: no access leaves a plane.
// The double-buffered sad[] needs one barrier an item: item i + 2 writes the buffer of item i only after every thread
// has passed the barrier of item i + 1, that is after its reads of item i.
// Statistics (optional): {moving blocks, blocks, sum m luma, sum m chroma} per frame. A thread keeps the sums of the
// frame it works on and adds them to memory (one atomic a wave and word, picture_dev.h's wave_add_counters) when the
// frame changes and at the end.
//
// A translation unit and a code object of its own, as orient.hip is: the library's other kernels stay byte for byte
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
#define H264MI_DENOISE_STRIP 256  // luma samples across a strip

struct DenoiseLaunch {
    const uint8_t *cur, *prev;
    uint8_t *dst, *dst2;   // dst2 may be null
    uint32_t *stats;       // 4 words a frame, or null
    size_t fb;             // frame f of each: base + f * fb
    size_t off[3];         // a frame's planes
    int w, h, n;
    int nsx, nsy;          // strips across, strip rows
    int motion;
    long long items, per;  // n * nsx * nsy; items a block
    DenoiseTables tab;
};

// one dword of a static block: O from C and P, the sum of m added to *sum
PICDEV uint32_t denoise_dword(uint32_t c4, uint32_t p4, const uint8_t *mt, uint32_t *sum) {
    if (c4 == p4) return c4;
    uint32_t o4 = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int c = (c4 >> (8 * j)) & 255, p = (p4 >> (8 * j)) & 255;
        const int d = c - p, a = d < 0 ? -d : d;
        const int m = a < 32 ? mt[a] : 0;
        *sum += (uint32_t)m;
        o4 |= (uint32_t)(d < 0 ? c + m : c - m) << (8 * j);
    }
    return o4;
}

__global__ __launch_bounds__(256) void denoise_kernel(DenoiseLaunch a) {
    __shared__ uint32_t sad[2][8][32];
    __shared__ uint32_t ktab[16];   // k[2][32] as bytes
    __shared__ uint8_t mtab[2][32]; // m = (a k + 128) >> 8
    const int t = threadIdx.x, b = t & 31, lr = t >> 5, pl = t >> 7, cr = (t >> 5) & 3;
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < 16; k++) ktab[k] = a.tab.k[k];
    }
    __syncthreads();
    if (t < 64) mtab[t >> 5][b] = (uint8_t)((b * (int)((const uint8_t *)ktab)[t] + 128) >> 8);
    __syncthreads();

    const int cw = a.w >> 1, chh = a.h >> 1;
    const long long it0 = (long long)blockIdx.x * a.per, it1 = min(it0 + a.per, a.items);
    const int per_frame = a.nsx * a.nsy;
    long long sf = -1;                       // the frame of the sums below
    uint32_t s_mov = 0, s_blk = 0, s_y = 0, s_c = 0;
    int par = 0;
    for (long long it = it0; it < it1; it++, par ^= 1) {  // the same count in every thread of a block
        const long long f = it / per_frame;
        const int k = (int)(it - f * per_frame);
        const int sy = k / a.nsx, sx = k - sy * a.nsx;
        if (a.stats && f != sf) {
            if (sf >= 0) {
                wave_add_counters(a.stats + 4 * sf, t & 63, s_mov, s_blk, s_y, s_c);
            }
            sf = f; s_mov = s_blk = s_y = s_c = 0;
        }
        const size_t fo = (size_t)f * a.fb;
        // ---- loads: everything this thread reads of the item
        const int x = sx * H264MI_DENOISE_STRIP + 8 * b, y = sy * 8 + lr;
        const bool ly = x < a.w && y < a.h;
        const int nby = ly ? min(8, a.w - x) : 0;
        const size_t yo = fo + (size_t)y * a.w + x;
        const bool wide_y = ((((uintptr_t)(a.cur + fo)) | ((uintptr_t)(a.prev + fo)) | ((uintptr_t)(a.dst + fo)) |
                              (a.dst2 ? (uintptr_t)(a.dst2 + fo) : 0) | (uintptr_t)a.w) & 7) == 0;  // then nby is 0 or 8
        uint32_t c0 = 0, c1 = 0, p0 = 0, p1 = 0;
        if (ly) {
            if (wide_y) {
                const uint2 cv = *(const uint2 *)(a.cur + yo), pv = *(const uint2 *)(a.prev + yo);
                c0 = cv.x; c1 = cv.y; p0 = pv.x; p1 = pv.y;
            } else {
                const uint8_t *cp = a.cur + yo, *pp = a.prev + yo;
                for (int j = 0; j < nby; j++) {
                    const uint32_t cb = (uint32_t)cp[j] << (8 * (j & 3)), pb = (uint32_t)pp[j] << (8 * (j & 3));
                    if (j < 4) { c0 |= cb; p0 |= pb; } else { c1 |= cb; p1 |= pb; }
                }
            }
        }
        const int cx = sx * (H264MI_DENOISE_STRIP / 2) + 4 * b, cy = sy * 4 + cr;
        const bool lc = cx < cw && cy < chh;
        const int nbc = lc ? min(4, cw - cx) : 0;
        const size_t co = fo + a.off[1 + pl] + (size_t)cy * cw + cx;
        const size_t cbase = fo + a.off[1 + pl];
        const bool wide_c = ((((uintptr_t)(a.cur + cbase)) | ((uintptr_t)(a.prev + cbase)) | ((uintptr_t)(a.dst + cbase)) |
                              (a.dst2 ? (uintptr_t)(a.dst2 + cbase) : 0) | (uintptr_t)cw) & 3) == 0;  // then nbc is 0 or 4
        uint32_t cc = 0, pc = 0;
        if (lc) {
            if (wide_c) {
                cc = *(const uint32_t *)(a.cur + co); pc = *(const uint32_t *)(a.prev + co);
            } else {
                for (int j = 0; j < nbc; j++) { cc |= (uint32_t)a.cur[co + j] << (8 * j); pc |= (uint32_t)a.prev[co + j] << (8 * j); }
            }
        }
        // ---- the gate: the row's SAD (bytes beyond the row are 0 on both sides), the block's eight rows through LDS
        sad[par][lr][b] = __builtin_amdgcn_sad_u8(c1, p1, __builtin_amdgcn_sad_u8(c0, p0, 0u));
        __syncthreads();  // the last read of the item's blocks lies in front of this barrier, every write behind it
        uint32_t bs = 0;
#pragma unroll
        for (int r = 0; r < 8; r++) bs += sad[par][r][b];
        const int bx0 = sx * H264MI_DENOISE_STRIP + 8 * b;
        const int npix = min(8, a.w - bx0) * min(8, a.h - sy * 8);  // of no meaning beyond the frame's edge: no lane there uses it
        const bool moving = 4 * bs > (uint32_t)(a.motion * npix);
        if (lr == 0 && bx0 < a.w) { s_blk++; s_mov += moving ? 1u : 0u; }
        // ---- the sample rule and the stores
        if (ly) {
            uint32_t o0 = c0, o1 = c1;
            if (!moving) { o0 = denoise_dword(c0, p0, mtab[0], &s_y); o1 = denoise_dword(c1, p1, mtab[0], &s_y); }
            if (wide_y) {
                *(uint2 *)(a.dst + yo) = make_uint2(o0, o1);
                if (a.dst2) *(uint2 *)(a.dst2 + yo) = make_uint2(o0, o1);
            } else {
                for (int j = 0; j < nby; j++) {
                    const uint8_t v = (uint8_t)((j < 4 ? o0 : o1) >> (8 * (j & 3)));
                    a.dst[yo + j] = v;
                    if (a.dst2) a.dst2[yo + j] = v;
                }
            }
        }
        if (lc) {
            const uint32_t oc = moving ? cc : denoise_dword(cc, pc, mtab[1], &s_c);
            if (wide_c) {
                *(uint32_t *)(a.dst + co) = oc;
                if (a.dst2) *(uint32_t *)(a.dst2 + co) = oc;
            } else {
                for (int j = 0; j < nbc; j++) {
                    a.dst[co + j] = (uint8_t)(oc >> (8 * j));
                    if (a.dst2) a.dst2[co + j] = (uint8_t)(oc >> (8 * j));
                }
            }
        }
    }
    if (a.stats && sf >= 0) {
        wave_add_counters(a.stats + 4 * sf, t & 63, s_mov, s_blk, s_y, s_c);
    }
}

// ---- host
// the definition on the host, one frame, as plain loops: out, cur and prev are tight w x h frames (out may be cur or
// prev: a block is read whole before it is written); stats, when given, receives the frame's four words
void denoise_frame_host(uint8_t *out, const uint8_t *cur, const uint8_t *prev, int w, int h, const h264mi_denoise &p, uint32_t *stats) {
    const size_t off[3] = {0, (size_t)w * h, (size_t)w * h + (size_t)(w / 2) * (h / 2)};
    uint32_t st[4] = {0, 0, 0, 0};
    for (int by = 0; 8 * by < h; by++)
        for (int bx = 0; 8 * bx < w; bx++) {
            const int bw = std::min(8, w - 8 * bx), bh = std::min(8, h - 8 * by);
            int sad = 0;
            for (int y = 0; y < bh; y++)
                for (int x = 0; x < bw; x++) {
                    const size_t i = (size_t)(8 * by + y) * w + 8 * bx + x;
                    sad += abs((int)cur[i] - (int)prev[i]);
                }
            const bool moving = 4 * sad > p.motion * bw * bh;
            st[0] += moving; st[1]++;
            for (int pl = 0; pl < 3; pl++) {
                const int pw = pl ? w / 2 : w, x0 = pl ? 4 * bx : 8 * bx, y0 = pl ? 4 * by : 8 * by;
                const int rw = pl ? bw / 2 : bw, rh = pl ? bh / 2 : bh, K = pl ? p.strength_c : p.strength_y;
                for (int y = 0; y < rh; y++)
                    for (int x = 0; x < rw; x++) {
                        const size_t i = off[pl] + (size_t)(y0 + y) * pw + x0 + x;
                        const int c = cur[i], d = c - (int)prev[i], a = abs(d);
                        const int m = moving ? 0 : (a * denoise_k(K, p.reach, a) + 128) >> 8;
                        st[pl ? 3 : 2] += (uint32_t)m;
                        out[i] = (uint8_t)(d < 0 ? c + m : c - m);
                    }
            }
        }
    if (stats) memcpy(stats, st, sizeof st);
}
// n tight w x h I420 frames: arguments as denoise_args_ok accepts them. One memset (with statistics) and one launch
int launch_denoise_i420(uint8_t *dst, uint8_t *dst2, const uint8_t *cur, const uint8_t *prev, int w, int h, int n, const h264mi_denoise &p,
                        uint32_t *stats, hipStream_t s) {
    const size_t ly = (size_t)w * h, lc = (size_t)(w / 2) * (h / 2);
    DenoiseLaunch a{};
    a.cur = cur; a.prev = prev; a.dst = dst; a.dst2 = dst2; a.stats = stats;
    a.fb = ly + 2 * lc;
    a.off[0] = 0; a.off[1] = ly; a.off[2] = ly + lc;
    a.w = w; a.h = h; a.n = n;
    a.nsx = (w + H264MI_DENOISE_STRIP - 1) / H264MI_DENOISE_STRIP;
    a.nsy = (h + 7) / 8;
    a.motion = p.motion;
    a.items = (long long)n * a.nsx * a.nsy;
    const long long blocks = std::min(a.items, (long long)PIC_MAX_BLOCKS);
    a.per = (a.items + blocks - 1) / blocks;
    denoise_tables(&a.tab, p);
    if (stats && hipMemsetAsync(stats, 0, 16 * (size_t)n, s) != hipSuccess) return -1;
    (void)hipGetLastError();
    hipLaunchKernelGGL(denoise_kernel, dim3((unsigned)((a.items + a.per - 1) / a.per)), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace h264mi
