// scenecut.hip -- the scene-cut detector of tight I420 frames on the device (gfx950) and the encoder's key-frame
// decision, as include/h264mi.h (h264mi_i420_scenecut_dev, h264mi_enc_set_scenecut) defines them. DESIGN.md §5.14.
//   scenecut_kernel        : n frames of one geometry per launch -- the standalone call, or an encoder's input area
//                            against its thumbnail state
//   scenecut_decide_kernel : one thread per stream: the policy's decision, written into EncState::force_idr
// The rule. Luma is cut into 4 x 4 cells (2 or 4 wide and high at the right and lower edge); a cell's thumbnail byte is
// T = (sum + npix / 2) / npix. The thumbnail is cut into blocks of 8 x 8 cells (smaller ones at the edge, ncell cells).
//   block:  sad = sum |Tc - Tp|, dsum = |sum Tc - sum Tp|, m = compensate ? sad - dsum : sad;
//           changed iff 4 m > level * ncell
//   frame:  {changed, blocks, sum sad, sum Tc, sum Tp, 0, 0, 0}; cut iff 256 changed > share * blocks
//
// Work split. A block of four waves owns one item: one row of thumbnail blocks -- 32 luma rows -- by a strip of 512
// luma samples (16 thumbnail blocks) of one frame. The items (frame, block row, strip) are dealt to the blocks in runs
// of consecutive items; the loop count depends on the block only, so the barrier is uniform.
//   luma:   thread t holds the 16 bytes x = 16 (t & 31) .. + 15 of the four rows of cell row t >> 5: four cells. 32
//           consecutive lanes load 512 consecutive bytes of a row, a wave eight rows. Each byte is read once.
//   cells:  a dword of a row is a cell's row: v_sad_u8 against zero adds it to the cell's sum. Bytes beyond the row
//           count as 0, rows beyond the frame are not added.
//   block:  a thread's four Tc and Tp bytes give sad, sum Tc and sum Tp by three more v_sad_u8; the sixteen threads of
//           a thumbnail block (two of each of eight cell rows, in all four waves) meet in LDS (one barrier), and
//           thread b < 16 sums block b of the strip.
// THE ALIASING INVARIANT. d_thumb_out may be exactly d_thumb_prev. A thread reads the Tp bytes of its own four cells
// into a register and later writes its Tc bytes to exactly those addresses; no other thread of the launch reads or
// writes them (cells of different threads and blocks of different items share no byte). So in place is safe thread by
// thread, whatever the order of the threads. Every read of a block still comes in front of the item's barrier and
// every write behind it, but the barrier is there for the LDS exchange of the statistics alone: without d_stats there
// is none.
// Two paths for the same bytes, chosen per frame from the frame's own pointers and row length: luma whose base and w are
// multiples of 16 moves as 16-byte words, a thumbnail whose bases and tw are multiples of 4 as dwords; any other (a
// buffer at an odd address, a row of 34 bytes) moves as bytes, gathered into the same registers. An aligned word of a
// row whose length is a multiple of the word never leaves the row, the byte path stops at the row's end: no access
// leaves a plane.
// The double-buffered part[] needs one barrier an item: item i + 2 writes the buffer of item i only after every thread
// has passed the barrier of item i + 1, that is after its reads of item i.
// Statistics: a thread keeps the sums of the frame it works on and adds them to memory (one atomic a wave and word,
// none for a zero: picture_dev.h's wave_add_counters) when the frame changes and at the end.
//
// A translation unit and a code object of its own, as denoise.hip is: the library's other kernels stay byte for byte
// what they were. The host runtime (enc_input.inc, capi_enc.inc) reaches it through the functions picture_host.h declares.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/h264mi.h"
#include "h264mi_types.h"
#include "picture_host.h"
#include "picture_dev.h"

namespace h264mi {
#define H264MI_SCENECUT_STRIP 512  // luma samples across a strip: 128 cells, 16 thumbnail blocks

struct ScenecutLaunch {
    const uint8_t *cur, *tprev;  // tprev may be null: thumbnails only
    uint8_t *tout;               // may be null, may be tprev
    uint32_t *stats;             // 8 words a frame, or null
    size_t fb, tb;               // frame f: cur + f * fb, thumbnails + f * tb
    int w, h, tw, th, n;
    int nsx, nby;                // strips across, block rows
    int level, compensate;
    long long items, per;        // n * nsx * nby; items a block
};

__global__ __launch_bounds__(256) void scenecut_kernel(ScenecutLaunch a) {
    __shared__ uint32_t part[2][3][8][32];  // sad, sum Tc, sum Tp of a thread's four cells: [cell row][16-byte column]
    const int t = threadIdx.x, q = t & 31, cr = t >> 5;
    const long long it0 = (long long)blockIdx.x * a.per, it1 = min(it0 + a.per, a.items);
    const int per_frame = a.nsx * a.nby;
    long long sf = -1;  // the frame of the sums below
    uint32_t s_chg = 0, s_blk = 0, s_sad = 0, s_tc = 0, s_tp = 0;
    int par = 0;
    for (long long it = it0; it < it1; it++, par ^= 1) {  // the same count in every thread of a block
        const long long f = it / per_frame;
        const int k = (int)(it - f * per_frame);
        const int by = k / a.nsx, sx = k - by * a.nsx;
        if (a.stats && f != sf) {
            if (sf >= 0) wave_add_counters(a.stats + 8 * sf, t & 63, s_chg, s_blk, s_sad, s_tc, s_tp);
            sf = f; s_chg = s_blk = s_sad = s_tc = s_tp = 0;
        }
        const uint8_t *cf = a.cur + (size_t)f * a.fb;
        const size_t to = (size_t)f * a.tb;
        // ---- loads: everything this thread reads of the item
        const int x = sx * H264MI_SCENECUT_STRIP + 16 * q, y0 = by * 32 + 4 * cr;
        const int cx0 = x >> 2, cy = y0 >> 2;
        const bool in = x < a.w && y0 < a.h;
        const int nr = in ? min(4, a.h - y0) : 0;   // 2 or 4 rows
        const int nbx = in ? min(16, a.w - x) : 0;  // bytes of a row, even
        const int ncx = (nbx + 3) >> 2;             // cells
        const bool wide = ((((uintptr_t)cf) | (uintptr_t)a.w) & 15) == 0;  // then nbx is 0 or 16
        const bool wide_t = ((((uintptr_t)(a.tprev ? a.tprev + to : nullptr)) | ((uintptr_t)(a.tout ? a.tout + to : nullptr)) |
                              (uintptr_t)a.tw) & 3) == 0;                  // then ncx is 0 or 4
        uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, tp4 = 0;
        if (in) {
            if (wide) {
                // rows 0 and 1 exist (h is even); rows 2 and 3 are loaded from a row that does and not added
                const uint4 *p0 = (const uint4 *)(cf + (size_t)y0 * a.w + x);
                const size_t step = nr == 4 ? (size_t)a.w : 0;
                const uint4 v0 = *p0, v1 = *(const uint4 *)((const uint8_t *)p0 + a.w);
                const uint4 v2 = *(const uint4 *)((const uint8_t *)p0 + 2 * step), v3 = *(const uint4 *)((const uint8_t *)p0 + 3 * step);
                s0 = __builtin_amdgcn_sad_u8(v1.x, 0u, __builtin_amdgcn_sad_u8(v0.x, 0u, 0u));
                s1 = __builtin_amdgcn_sad_u8(v1.y, 0u, __builtin_amdgcn_sad_u8(v0.y, 0u, 0u));
                s2 = __builtin_amdgcn_sad_u8(v1.z, 0u, __builtin_amdgcn_sad_u8(v0.z, 0u, 0u));
                s3 = __builtin_amdgcn_sad_u8(v1.w, 0u, __builtin_amdgcn_sad_u8(v0.w, 0u, 0u));
                if (nr == 4) {
                    s0 = __builtin_amdgcn_sad_u8(v3.x, 0u, __builtin_amdgcn_sad_u8(v2.x, 0u, s0));
                    s1 = __builtin_amdgcn_sad_u8(v3.y, 0u, __builtin_amdgcn_sad_u8(v2.y, 0u, s1));
                    s2 = __builtin_amdgcn_sad_u8(v3.z, 0u, __builtin_amdgcn_sad_u8(v2.z, 0u, s2));
                    s3 = __builtin_amdgcn_sad_u8(v3.w, 0u, __builtin_amdgcn_sad_u8(v2.w, 0u, s3));
                }
            } else {
                for (int r = 0; r < nr; r++) {
                    const uint8_t *row = cf + (size_t)(y0 + r) * a.w + x;
                    for (int j = 0; j < nbx; j++) {
                        const uint32_t v = row[j];
                        if (j < 4) s0 += v; else if (j < 8) s1 += v; else if (j < 12) s2 += v; else s3 += v;
                    }
                }
            }
            if (a.tprev) {
                const uint8_t *pp = a.tprev + to + (size_t)cy * a.tw + cx0;
                if (wide_t) tp4 = *(const uint32_t *)pp;
                else for (int j = 0; j < ncx; j++) tp4 |= (uint32_t)pp[j] << (8 * j);
            }
        }
        // ---- the cells' thumbnail bytes: a cell of the thread is 4 wide but the last one of a row that ends on 2
        const int sh_y = nr == 4 ? 2 : 1;
        const int last = ncx - 1, sh_last = (nbx & 3) ? sh_y + 1 : sh_y + 2;
        uint32_t tc4 = 0;
        {
            const uint32_t sum[4] = {s0, s1, s2, s3};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int sh = j == last ? sh_last : sh_y + 2;
                if (j < ncx) tc4 |= ((sum[j] + (1u << (sh - 1))) >> sh) << (8 * j);
            }
        }
        // ---- the block's sums: cells beyond the frame are 0 on both sides
        if (a.stats) {  // uniform over the launch; statistics come with previous thumbnails only
            part[par][0][cr][q] = __builtin_amdgcn_sad_u8(tc4, tp4, 0u);
            part[par][1][cr][q] = __builtin_amdgcn_sad_u8(tc4, 0u, 0u);
            part[par][2][cr][q] = __builtin_amdgcn_sad_u8(tp4, 0u, 0u);
            __syncthreads();  // for part[]; the last read of the item's blocks lies in front of it, every write behind it
        }
        if (in && a.tout) {
            uint8_t *op = a.tout + to + (size_t)cy * a.tw + cx0;
            if (wide_t) *(uint32_t *)op = tc4;
            else for (int j = 0; j < ncx; j++) op[j] = (uint8_t)(tc4 >> (8 * j));
        }
        if (a.stats && t < 16) {
            const int bx = sx * (H264MI_SCENECUT_STRIP / 32) + t;
            if (8 * bx < a.tw) {
                uint32_t sad = 0, sc = 0, sp = 0;
#pragma unroll
                for (int r = 0; r < 8; r++) {
                    sad += part[par][0][r][2 * t] + part[par][0][r][2 * t + 1];
                    sc += part[par][1][r][2 * t] + part[par][1][r][2 * t + 1];
                    sp += part[par][2][r][2 * t] + part[par][2][r][2 * t + 1];
                }
                const uint32_t ncell = (uint32_t)(min(8, a.tw - 8 * bx) * min(8, a.th - 8 * by));
                const uint32_t dsum = sc > sp ? sc - sp : sp - sc;
                const uint32_t m = a.compensate ? sad - dsum : sad;
                s_blk++;
                s_chg += 4 * m > (uint32_t)a.level * ncell ? 1u : 0u;
                s_sad += sad; s_tc += sc; s_tp += sp;
            }
        }
    }
    if (a.stats && sf >= 0) wave_add_counters(a.stats + 8 * sf, t & 63, s_chg, s_blk, s_sad, s_tc, s_tp);
}

// the policy of include/h264mi.h for S streams, one thread each. words: a stream's sixteen -- the frame's eight
// statistics words, then {cut, key, reason, dist, keys by cut, by period, other, frames}
struct ScenecutDecide {
    EncState *st;
    uint32_t *words;
    const uint32_t *stats;  // 8 a stream, or null: no detector ran for this frame
    int S, share, min_gap, max_gap;
};

__global__ __launch_bounds__(64) void scenecut_decide_kernel(ScenecutDecide a) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.S) return;
    EncState *st = a.st + s;
    uint32_t *wd = a.words + 16 * (size_t)s;
    uint32_t sv[8];
#pragma unroll
    for (int k = 0; k < 8; k++) sv[k] = a.stats ? a.stats[8 * (size_t)s + k] : 0u;
    const uint32_t dist1 = wd[11] + 1;
    const bool other = st->first || st->force_idr || st->err != 0;
    const bool period = a.max_gap > 0 && dist1 >= (uint32_t)a.max_gap;
    const bool cut = a.stats && scenecut_is_cut(a.share, sv[0], sv[1]) && dist1 >= (uint32_t)a.min_gap;
    const bool key = other || period || cut;
    const uint32_t reason = other ? 3u : period ? 2u : cut ? 1u : 0u;
    if (key) st->force_idr = 1;
#pragma unroll
    for (int k = 0; k < 8; k++) wd[k] = sv[k];
    wd[8] = cut; wd[9] = key; wd[10] = reason;
    wd[11] = key ? 0u : dist1;
    if (reason == 1) wd[12] = wd[12] + 1;
    if (reason == 2) wd[13] = wd[13] + 1;
    if (reason == 3) wd[14] = wd[14] + 1;
    wd[15] = wd[15] + 1;
}

// ---- host
// the definition on the host, one frame, as plain loops: cur a tight w x h frame; thumb_out (tw x th bytes; may be
// thumb_prev: a block is read whole before it is written; may be null) receives the thumbnail; stats, when given
// (thumb_prev then too), the frame's eight words
void scenecut_frame_host(uint32_t *stats, uint8_t *thumb_out, const uint8_t *cur, const uint8_t *thumb_prev, int w, int h, const h264mi_scenecut &p) {
    const int tw = thumb_side(w), th = thumb_side(h);
    uint32_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int by = 0; 8 * by < th; by++)
        for (int bx = 0; 8 * bx < tw; bx++) {
            const int bw = std::min(8, tw - 8 * bx), bh = std::min(8, th - 8 * by);
            uint8_t tc[64];
            uint32_t sad = 0, sc = 0, sp = 0;
            for (int y = 0; y < bh; y++)
                for (int x = 0; x < bw; x++) {
                    const int cx = 8 * bx + x, cy = 8 * by + y;
                    const int cw = std::min(4, w - 4 * cx), ch = std::min(4, h - 4 * cy);
                    uint32_t sum = 0;
                    for (int j = 0; j < ch; j++)
                        for (int i = 0; i < cw; i++) sum += cur[(size_t)(4 * cy + j) * w + 4 * cx + i];
                    const uint32_t T = (sum + (uint32_t)(cw * ch) / 2) / (uint32_t)(cw * ch);
                    tc[8 * y + x] = (uint8_t)T;
                    sc += T;
                    if (thumb_prev) {
                        const uint32_t P = thumb_prev[(size_t)cy * tw + cx];
                        sp += P;
                        sad += T > P ? T - P : P - T;
                    }
                }
            if (thumb_out)
                for (int y = 0; y < bh; y++)
                    for (int x = 0; x < bw; x++) thumb_out[(size_t)(8 * by + y) * tw + 8 * bx + x] = tc[8 * y + x];
            const uint32_t dsum = sc > sp ? sc - sp : sp - sc;
            const uint32_t m = p.compensate ? sad - dsum : sad;
            st[0] += 4 * m > (uint32_t)p.level * (uint32_t)(bw * bh);
            st[1]++;
            st[2] += sad; st[3] += sc; st[4] += sp;
        }
    if (stats && thumb_prev) memcpy(stats, st, sizeof st);
}
// n tight w x h I420 frames: arguments as scenecut_args_ok accepts them. One memset (with statistics) and one launch
int launch_scenecut_i420(uint32_t *stats, uint8_t *thumb_out, const uint8_t *cur, const uint8_t *thumb_prev, int w, int h, int n,
                         const h264mi_scenecut &p, hipStream_t s) {
    ScenecutLaunch a{};
    a.cur = cur; a.tprev = thumb_prev; a.tout = thumb_out; a.stats = stats;
    a.fb = i420_bytes(w, h); a.tb = thumb_bytes(w, h);
    a.w = w; a.h = h; a.tw = thumb_side(w); a.th = thumb_side(h); a.n = n;
    a.nsx = (w + H264MI_SCENECUT_STRIP - 1) / H264MI_SCENECUT_STRIP;
    a.nby = (h + 31) / 32;
    a.level = p.level; a.compensate = p.compensate;
    a.items = (long long)n * a.nsx * a.nby;
    const long long blocks = std::min(a.items, (long long)PIC_MAX_BLOCKS);
    a.per = (a.items + blocks - 1) / blocks;
    if (stats && hipMemsetAsync(stats, 0, 32 * (size_t)n, s) != hipSuccess) return -1;
    (void)hipGetLastError();
    hipLaunchKernelGGL(scenecut_kernel, dim3((unsigned)((a.items + a.per - 1) / a.per)), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int launch_scenecut_decide(EncState *st, uint32_t *words, const uint32_t *stats, int S, const h264mi_scenecut &p, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(scenecut_decide_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, s,
                       ScenecutDecide{st, words, stats, S, p.share, p.min_gap, p.max_gap});
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace h264mi
