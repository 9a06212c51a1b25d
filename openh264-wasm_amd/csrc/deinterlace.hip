// deinterlace.hip -- the deinterlacer of tight I420 frames on the device (gfx950), as include/h264mi.h
// (h264mi_i420_deinterlace_dev) defines it. DESIGN.md §5.15.
//   deinterlace_kernel : n frames of one geometry per launch -- the standalone call, or an encoder's input area
//                        filtered in place against its state (h264mi_enc_set_deinterlace)
// The rule, for each of the three planes on its own (pw x ph). C is the current frame, P the previous unfiltered one
// (optional), O the output. Lines y % 2 == parity are kept: O = C. A missing line y has up = C[y-1], dn = C[y+1]:
//   linear:        s = (up[x] + dn[x] + 1) >> 1
//   edge-directed: score_d = sum j = -1..1 |up[cx(x+j+d)] - dn[cx(x+j-d)]| for d = 0, -1, +1 (the smallest wins, a tie
//                  goes to the earlier), s = (up[cx(x+d)] + dn[cx(x-d)] + 1) >> 1
//   one neighbour: s = its sample at x; none (ph == 1, parity 1): O = C
//   temporal with P: k = y ^ 1 (y if outside), m = max(|C[y][x] - P[y][x]|, |C[k][x] - P[k][x]|),
//                  O = min(max(s, v - m), v + m), v = C[y][x]; otherwise O = s
//
// Work split. The unit is the line pair (2j, 2j+1) of a plane: one missing line, one kept line. A block of four waves
// owns one item: a row group of 16 rows (8 line pairs) x a strip of 256 samples of one plane of one frame. Thread t
// holds the 8 bytes x = 8 (t & 31) .. + 7 of line pair t >> 5: 32 consecutive lanes load and store 256 consecutive
// bytes of a row, a wave two line pairs. The items (frame, plane, row group, strip) are dealt to the blocks in runs of
// consecutive items; the loop count depends on the block only, so every lane of a wave reaches the lane exchanges.
// A thread loads the 8 bytes of its missing line, of up and of dn (one of them its pair's kept line), with P the same
// 8 bytes of P's two lines. The edge-directed taps at x - 2 .. x + 9 come from the neighbouring lanes' registers; the
// first and the last lane of a row, whose neighbour holds another row, load them (a dword inside the row), and at
// the row's two ends they are the clamped edge sample. The three-sample scores are v_sad_u8 of dwords shifted out of
// that window with the fourth byte masked. No LDS, no barrier.
// THE ALIASING INVARIANT. d_dst may be exactly d_cur: kept lines are then not written at all, and a thread reads its
// own v before it writes O there; every other byte it reads of C lies on a kept line. d_prev_out may be exactly
// d_prev: it receives the unfiltered C, and a thread reads P only at the bytes of its own line pair and columns,
// which are the bytes it later writes. Any other overlap of a written with a read range the host refuses
// (deinterlace_args_ok); d_prev may overlap d_cur when neither is written.
// Two paths for the same bytes, chosen per plane and frame from the plane's own pointers and row length: a plane
// whose bases (of every buffer in the call) and pw are multiples of 8 moves as 8-byte words (its halo as aligned
// dwords), any other plane as bytes gathered into the same registers. An aligned word of a row whose length is a
// multiple of the word never leaves the row, the byte path stops at the row's end: no access leaves a plane.
// Statistics (optional): {missing luma samples, combed luma samples, sum |O - v| luma, sum |O - v| chroma} per frame.
// A thread keeps the sums of the frame it works on and adds them to memory (one atomic a wave and word) when the
// frame changes and at the end.
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
#define H264MI_DEINT_STRIP 256  // samples across a strip
#define H264MI_DEINT_ROWS 16    // rows of a row group: 8 line pairs

struct DeintLaunch {
    const uint8_t *cur, *prev;  // prev may be null
    uint8_t *dst, *prev_out;    // prev_out may be null
    uint32_t *stats;            // 4 words a frame, or null
    size_t fb;                  // frame f of each: base + f * fb
    size_t off1, off2;          // a frame's chroma planes
    int w, h, n;
    int nsx_y, nsx_c;           // strips across the luma plane, a chroma plane
    int items_y, items_c;       // items of the luma plane, of one chroma plane
    int parity, edge, temporal, comb;
    long long items, per;       // n * (items_y + 2 items_c); items a block
};

struct Seg { uint32_t lo, hi; };

// the nb <= 8 bytes at p: one 8-byte word (nb == 8, p a multiple of 8) or bytes
PICDEV Seg load_seg(const uint8_t *p, int nb, bool wide) {
    Seg s{0, 0};
    if (wide) {
        const uint2 v = *(const uint2 *)p;
        s.lo = v.x; s.hi = v.y;
    } else {
        for (int j = 0; j < nb; j++) {
            const uint32_t v = (uint32_t)p[j] << (8 * (j & 3));
            if (j < 4) s.lo |= v; else s.hi |= v;
        }
    }
    return s;
}
PICDEV void store_seg(uint8_t *p, uint32_t lo, uint32_t hi, int nb, bool wide) {
    if (wide) {
        *(uint2 *)p = make_uint2(lo, hi);
    } else {
        for (int j = 0; j < nb; j++) p[j] = (uint8_t)((j < 4 ? lo : hi) >> (8 * (j & 3)));
    }
}
// bytes nb .. 7 of a segment take the value of byte nb - 1 (the clamp at a row's end); returns that byte four times
PICDEV uint32_t fill_tail(Seg &s, int nb) {
    const uint32_t rep = (((nb > 4 ? s.hi : s.lo) >> (8 * ((nb - 1) & 3))) & 255u) * 0x01010101u;
    if (nb < 4) {
        const uint32_t m = (1u << (8 * nb)) - 1u;
        s.lo = (s.lo & m) | (rep & ~m);
        s.hi = rep;
    } else if (nb == 4) {
        s.hi = rep;
    } else if (nb < 8) {
        const uint32_t m = (1u << (8 * (nb - 4))) - 1u;
        s.hi = (s.hi & m) | (rep & ~m);
    }
    return rep;
}
// the two bytes in front of a segment at row[x0], x0 >= 8, in the upper half of a dword
PICDEV uint32_t load_left(const uint8_t *row, int x0, bool wide) {
    if (wide) return *(const uint32_t *)(row + x0 - 4);
    return ((uint32_t)row[x0 - 2] << 16) | ((uint32_t)row[x0 - 1] << 24);
}
// the two bytes behind a segment, x0 + 8 < pw, clamped to the row, in the lower half of a dword
PICDEV uint32_t load_right(const uint8_t *row, int x0, int pw, bool wide) {
    if (wide) return *(const uint32_t *)(row + x0 + 8);
    return (uint32_t)row[x0 + 8] | ((uint32_t)row[min(x0 + 9, pw - 1)] << 8);
}
// a window of 16 bytes: W[0] the dword in front of the segment, W[1], W[2] the segment, W[3] the dword behind it.
// Three bytes from byte `pos` on (a constant after unrolling), the fourth masked; one byte
PICDEV uint32_t take3(const uint32_t (&W)[4], int pos) {
    const int q = pos >> 2, o = pos & 3;
    const uint32_t v = o ? (W[q] >> (8 * o)) | (W[q + 1] << (32 - 8 * o)) : W[q];
    return v & 0x00FFFFFFu;
}
PICDEV int byte_at(const uint32_t (&W)[4], int pos) { return (int)((W[pos >> 2] >> (8 * (pos & 3))) & 255u); }

__global__ __launch_bounds__(256) void deinterlace_kernel(DeintLaunch a) {
    const int t = threadIdx.x, b = t & 31, lr = t >> 5;
    const long long it0 = (long long)blockIdx.x * a.per, it1 = min(it0 + a.per, a.items);
    const int per_frame = a.items_y + 2 * a.items_c;
    const bool temporal = a.temporal && a.prev;
    long long sf = -1;  // the frame of the sums below
    uint32_t s_miss = 0, s_comb = 0, s_y = 0, s_c = 0;
    for (long long it = it0; it < it1; it++) {  // the same count in every thread of a block
        const long long f = it / per_frame;
        int k = (int)(it - f * per_frame), pl = 0;
        if (k >= a.items_y) {
            k -= a.items_y; pl = 1;
            if (k >= a.items_c) { k -= a.items_c; pl = 2; }
        }
        const int pw = pl ? a.w >> 1 : a.w, ph = pl ? a.h >> 1 : a.h, nsx = pl ? a.nsx_c : a.nsx_y;
        const int sy = k / nsx, sx = k - sy * nsx;
        if (a.stats && f != sf) {
            if (sf >= 0) {
                wave_add_counters(a.stats + 4 * sf, t & 63, s_miss, s_comb, s_y, s_c);
            }
            sf = f; s_miss = s_comb = s_y = s_c = 0;
        }
        const size_t po = (size_t)f * a.fb + (pl == 0 ? 0 : pl == 1 ? a.off1 : a.off2);  // the plane in each buffer
        const uint8_t *cp = a.cur + po, *pp = a.prev ? a.prev + po : nullptr;
        uint8_t *dp = a.dst + po, *qp = a.prev_out ? a.prev_out + po : nullptr;
        const bool wide = (((uintptr_t)cp | (uintptr_t)pp | (uintptr_t)dp | (uintptr_t)qp | (uintptr_t)pw) & 7) == 0;  // then nb is 0 or 8
        // ---- the thread's line pair and columns
        const int x0 = sx * H264MI_DEINT_STRIP + 8 * b, j = sy * (H264MI_DEINT_ROWS / 2) + lr;
        const bool in = x0 < pw && 2 * j < ph;
        const int nb = in ? min(8, pw - x0) : 0;
        const int ym = 2 * j + 1 - a.parity, yu = ym - 1, yd = ym + 1, yk = 2 * j + a.parity;  // yk is yu (parity 0) or yd
        const bool mv = in && ym < ph, uv = in && yu >= 0, dv = in && yd < ph, kv = a.parity ? dv : uv;
        // ---- loads: everything this thread reads of the item
        Seg U{0, 0}, D{0, 0}, V{0, 0}, PV{0, 0}, PK{0, 0};
        const uint8_t *urow = cp + (size_t)(uv ? yu : 0) * pw, *drow = cp + (size_t)(dv ? yd : 0) * pw;
        if (uv) U = load_seg(urow + x0, nb, wide);
        if (dv) D = load_seg(drow + x0, nb, wide);
        if (mv) V = load_seg(cp + (size_t)ym * pw + x0, nb, wide);
        const Seg K = kv ? (a.parity ? D : U) : V;  // the pair's kept line, or the missing line where there is none
        if (temporal && mv) {
            PV = load_seg(pp + (size_t)ym * pw + x0, nb, wide);
            PK = kv ? load_seg(pp + (size_t)yk * pw + x0, nb, wide) : PV;
        }
        uint32_t UL = 0, UR = 0, DL = 0, DR = 0;
        const bool last = in && x0 + 8 >= pw;  // the row ends in this segment: clamp
        if (last) { UR = fill_tail(U, nb); DR = fill_tail(D, nb); }
        if (a.edge) {  // the same in every lane
            const uint32_t ul = __shfl_up(U.hi, 1), ur = __shfl_down(U.lo, 1), dl = __shfl_up(D.hi, 1), dr = __shfl_down(D.lo, 1);
            if (in && x0 == 0) {
                UL = (U.lo & 255u) * 0x01010101u; DL = (D.lo & 255u) * 0x01010101u;
            } else if (b != 0) {
                UL = ul; DL = dl;
            } else if (in) {
                if (uv) UL = load_left(urow, x0, wide);
                if (dv) DL = load_left(drow, x0, wide);
            }
            if (!last) {
                if (b != 31) {
                    UR = ur; DR = dr;
                } else if (in) {
                    if (uv) UR = load_right(urow, x0, pw, wide);
                    if (dv) DR = load_right(drow, x0, pw, wide);
                }
            }
        }
        // ---- the rule
        uint32_t o[2] = {V.lo, V.hi};
        if (mv && (uv || dv)) {
            const bool both = uv && dv;
            const uint32_t WU[4] = {uv ? UL : DL, uv ? U.lo : D.lo, uv ? U.hi : D.hi, uv ? UR : DR};  // one neighbour: both are it
            const uint32_t WD[4] = {dv ? DL : UL, dv ? D.lo : U.lo, dv ? D.hi : U.hi, dv ? DR : UR};
            const uint32_t v2[2] = {V.lo, V.hi}, k2[2] = {K.lo, K.hi}, pv2[2] = {PV.lo, PV.hi}, pk2[2] = {PK.lo, PK.hi};
            uint32_t sum = 0;
#pragma unroll
            for (int hf = 0; hf < 2; hf++) {
                if (temporal && ((v2[hf] ^ pv2[hf]) | (k2[hf] ^ pk2[hf])) == 0) continue;  // m == 0 four times: woven
                uint32_t o4 = 0;
#pragma unroll
                for (int i = 4 * hf; i < 4 * hf + 4; i++) {
                    const int P = i + 4, sh = 8 * (i & 3);
                    int ua = byte_at(WU, P), da = byte_at(WD, P);
                    if (a.edge) {
                        uint32_t best = __builtin_amdgcn_sad_u8(take3(WU, P - 1), take3(WD, P - 1), 0u);
                        const uint32_t sm = __builtin_amdgcn_sad_u8(take3(WU, P - 2), take3(WD, P), 0u);
                        const uint32_t sp = __builtin_amdgcn_sad_u8(take3(WU, P), take3(WD, P - 2), 0u);
                        if (sm < best) { best = sm; ua = byte_at(WU, P - 1); da = byte_at(WD, P + 1); }
                        if (sp < best) { ua = byte_at(WU, P + 1); da = byte_at(WD, P - 1); }
                    }
                    int s = (ua + da + 1) >> 1;
                    const int v = (int)((v2[hf] >> sh) & 255u);
                    if (temporal) {
                        const int m0 = abs(v - (int)((pv2[hf] >> sh) & 255u));
                        const int m1 = abs((int)((k2[hf] >> sh) & 255u) - (int)((pk2[hf] >> sh) & 255u));
                        const int m = max(m0, m1);
                        s = min(max(s, v - m), v + m);
                    }
                    if (i < nb) sum += (uint32_t)abs(s - v);
                    o4 |= (uint32_t)s << sh;
                }
                o[hf] = o4;
            }
            if (pl) s_c += sum; else s_y += sum;
            if (a.stats && pl == 0) {
                s_miss += (uint32_t)nb;
                if (both) {
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        const int sh = 8 * (i & 3);
                        const int v = (int)((v2[i >> 2] >> sh) & 255u), du = v - byte_at(WU, i + 4), dd = v - byte_at(WD, i + 4);
                        const bool same = (du > 0 && dd > 0) || (du < 0 && dd < 0);
                        if (i < nb && same && min(abs(du), abs(dd)) > a.comb) s_comb++;
                    }
                }
            }
        }
        // ---- stores: O on the missing line; the kept line unless it is in place; the unfiltered pair to prev_out
        if (mv) {
            store_seg(dp + (size_t)ym * pw + x0, o[0], o[1], nb, wide);
            if (qp) store_seg(qp + (size_t)ym * pw + x0, V.lo, V.hi, nb, wide);
        }
        if (kv) {
            if (a.dst != a.cur) store_seg(dp + (size_t)yk * pw + x0, K.lo, K.hi, nb, wide);
            if (qp) store_seg(qp + (size_t)yk * pw + x0, K.lo, K.hi, nb, wide);
        }
    }
    if (a.stats && sf >= 0) {
        wave_add_counters(a.stats + 4 * sf, t & 63, s_miss, s_comb, s_y, s_c);
    }
}

// ---- host
// the definition on the host, one frame, sample by sample: out, cur and prev (may be null) are tight w x h frames. out
// may be cur: a missing sample is read before it is written and every other sample read lies on a kept line. stats,
// when given, receives the frame's four words
void deinterlace_frame_host(uint8_t *out, const uint8_t *cur, const uint8_t *prev, int w, int h, const h264mi_deinterlace &p, uint32_t *stats) {
    const size_t off[3] = {0, (size_t)w * h, (size_t)w * h + (size_t)(w / 2) * (h / 2)};
    uint32_t st[4] = {0, 0, 0, 0};
    for (int pl = 0; pl < 3; pl++) {
        const int pw = pl ? w / 2 : w, ph = pl ? h / 2 : h;
        const uint8_t *C = cur + off[pl], *P = prev ? prev + off[pl] : nullptr;
        uint8_t *O = out + off[pl];
        auto cx = [pw](int x) { return std::min(std::max(x, 0), pw - 1); };
        for (int y = 0; y < ph; y++) {
            const bool has_up = y >= 1, has_dn = y + 1 < ph;
            const uint8_t *row = C + (size_t)y * pw;
            if (y % 2 == p.parity || (!has_up && !has_dn)) {
                if (O != C) memcpy(O + (size_t)y * pw, row, (size_t)pw);
                continue;
            }
            const uint8_t *up = has_up ? row - pw : row + pw, *dn = has_dn ? row + pw : row - pw;  // one neighbour: both are it
            const int k = (y ^ 1) < ph ? (y ^ 1) : y;
            for (int x = 0; x < pw; x++) {
                const int v = row[x];
                int d = 0;
                if (p.spatial) {
                    int best = 0;
                    for (int c : {0, -1, 1}) {
                        int score = 0;
                        for (int j = -1; j <= 1; j++) score += abs((int)up[cx(x + j + c)] - (int)dn[cx(x + j - c)]);
                        if (c == 0 || score < best) { best = score; d = c; }
                    }
                }
                int s = ((int)up[cx(x + d)] + (int)dn[cx(x - d)] + 1) >> 1;
                if (p.temporal && P) {
                    const int m = std::max(abs(v - (int)P[(size_t)y * pw + x]), abs((int)C[(size_t)k * pw + x] - (int)P[(size_t)k * pw + x]));
                    s = std::min(std::max(s, v - m), v + m);
                }
                if (pl == 0) {
                    st[0]++;
                    if (has_up && has_dn) {
                        const int du = v - (int)up[x], dd = v - (int)dn[x];
                        if (((du > 0 && dd > 0) || (du < 0 && dd < 0)) && std::min(abs(du), abs(dd)) > p.comb_level) st[1]++;
                    }
                }
                st[pl ? 3 : 2] += (uint32_t)abs(s - v);
                O[(size_t)y * pw + x] = (uint8_t)s;
            }
        }
    }
    if (stats) memcpy(stats, st, sizeof st);
}
// n tight w x h I420 frames: arguments as deinterlace_args_ok accepts them. One memset (with statistics) and one launch
int launch_deinterlace_i420(uint8_t *dst, uint8_t *prev_out, const uint8_t *cur, const uint8_t *prev, int w, int h, int n,
                            const h264mi_deinterlace &p, uint32_t *stats, hipStream_t s) {
    const size_t ly = (size_t)w * h, lc = (size_t)(w / 2) * (h / 2);
    DeintLaunch a{};
    a.cur = cur; a.prev = prev; a.dst = dst; a.prev_out = prev_out; a.stats = stats;
    a.fb = ly + 2 * lc;
    a.off1 = ly; a.off2 = ly + lc;
    a.w = w; a.h = h; a.n = n;
    a.nsx_y = (w + H264MI_DEINT_STRIP - 1) / H264MI_DEINT_STRIP;
    a.nsx_c = (w / 2 + H264MI_DEINT_STRIP - 1) / H264MI_DEINT_STRIP;
    a.items_y = a.nsx_y * ((h + H264MI_DEINT_ROWS - 1) / H264MI_DEINT_ROWS);
    a.items_c = a.nsx_c * ((h / 2 + H264MI_DEINT_ROWS - 1) / H264MI_DEINT_ROWS);
    a.parity = p.parity; a.edge = p.spatial; a.temporal = p.temporal; a.comb = p.comb_level;
    a.items = (long long)n * (a.items_y + 2 * a.items_c);
    const long long blocks = std::min(a.items, (long long)PIC_MAX_BLOCKS);
    a.per = (a.items + blocks - 1) / blocks;
    if (stats && hipMemsetAsync(stats, 0, 16 * (size_t)n, s) != hipSuccess) return -1;
    (void)hipGetLastError();
    hipLaunchKernelGGL(deinterlace_kernel, dim3((unsigned)((a.items + a.per - 1) / a.per)), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace h264mi
