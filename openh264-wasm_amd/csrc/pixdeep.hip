// pixdeep.hip -- the deeper and wider pixel layouts to and from tight I420 on the device (gfx950): I422, I444, NV16, Y800,
// P010, I010, P210, I210 and V210 (ids 16..24), as include/h264mi.h (h264mi_pix_layout, h264mi_pixopt) defines them.
// DESIGN.md §5.17. The five formats of pixfmt.hip stay there, in their own code object.
//   pix_rows_kernel<deep_row_pair<false>>       : n frames in a layout -> n tight I420 frames (h264mi_pix_to_i420_opt_dev,
//                                                 h264mi_enc_encode_pix)
//   pix_rows_kernel<deep_row_pair<true>>        : n tight I420 frames -> n frames in a layout (h264mi_i420_to_pix_dev)
//   dec_output_rows_kernel<deep_row_pair<true>> : the batch decoder's per-frame read-out into a layout
// The kernels, their launchers, the frame, the 8-bit row move and byte average are pix_rows.h's, shared with pixfmt.hip;
// this file owns the row functions of its nine formats. One definition for all three kernels (deep_row_pair). The work split is §5.10's: a wave owns a row pair (luma rows 2r, 2r + 1,
// I420 chroma row r, and whatever rows of the layout hold them), a block of four waves a strip, blocks stride over
// (frame, strip); inside a row the lanes take consecutive pieces and loop.
//
// Access widths. The side with the most bytes per sample moves as 16 bytes a lane, the other in the widest access that
// holds the same samples:
//   8-bit planar rows (every Y but the deep ones; I422 chroma)   16 B in, 16 B out; the 4:2:2 average is pix_avg4's, per dword
//   I444 chroma      16 B of each of the two rows <-> 8 B of the I420 row. Both rows loaded, then the even and the odd
//                    bytes of a dword as two 16-bit fields each: four packed adds, +2, one packed shift, one v_perm_b32 per
//                    two dwords. The other way one dword is zipped with itself (two v_perm_b32), stored to both rows
//   NV16 chroma      16 B interleaved of each row <-> 8 B Cb + 8 B Cr; averaged while interleaved, split by v_perm_b32
//   16-bit planar (Y of P010/I010/P210/I210, Cb Cr of I010/I210)   16 B = 8 words <-> 8 B. Narrowing: the two words of a
//                    dword are two 16-bit fields: shift or mask to the 10-bit value, (4:2:2: packed add of the two rows,
//                    +1, >> 1,) packed add of the rounding or dither pair, packed >> 2, packed min 255, and one v_perm_b32
//                    takes the four low bytes of two dwords. Widening: v_perm_b32 puts each byte into the high byte of
//                    its word (v << 8 = (v << 2) << 6, the MSB formats) or the low one and one shift by 2 (the LSB formats)
//   16-bit interleaved (Cb Cr of P010/P210)   16 B = 4 Cb Cr pairs <-> 4 B Cb + 4 B Cr, the same arithmetic, then two
//                    rounds of v_perm_b32 to split. Dither: a dword holds one chroma position, so its pair is D D
//   V210             a lane owns a run of eight groups = 128 B = 48 luma samples a row, 24 Cb, 24 Cr: eight 16-byte loads
//                    a row on the packed side, three 16-byte stores a luma row and three 8-byte stores a chroma row.
//                    Fields are extracted with v_bfe_u32 and bytes assembled with v_lshl_or_b32 (DESIGN.md §5.17 counts
//                    them against staging through LDS). Groups past the last whole run, partial groups, and every group
//                    of a row that is not aligned go one group a lane: four dword accesses on the packed side, bytes on
//                    the other
// Two paths for the same values as in §5.10: wide when every pointer a piece touches is a multiple of its access width
// and the piece lies inside the row, the scalar path (units of the format: bytes, 16-bit words, V210's dwords) otherwise.
// Neither leaves the bytes the layout names; V210's row bytes, 16 * ceil(w / 6), are all named and all written.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include "../../include/h264mi.h"
#include "pix_rows.h"

namespace h264mi {
// v_perm_b32 selectors beside pix_rows.h's
#define DEEP_SEL_HIGH_LO 0x010c000cu   // (-, x) -> 0 x.0 0 x.1
#define DEEP_SEL_HIGH_HI 0x030c020cu   // (-, x) -> 0 x.2 0 x.3

typedef unsigned short deep_pk __attribute__((ext_vector_type(2)));  // two 16-bit fields of a dword: v_pk_* arithmetic
PICDEV deep_pk deep_as_pk(uint32_t x) { return __builtin_bit_cast(deep_pk, x); }
PICDEV uint32_t deep_as_u32(deep_pk x) { return __builtin_bit_cast(uint32_t, x); }

// the depth rule's addends for the output samples at even and odd x of output row y, as the fields of a dword
PICDEV uint32_t deep_addend(int depth, int y) {
    if (depth == H264MI_DEPTH_DITHER) return (y & 1) ? 0x00010003u : 0x00020000u;  // D = {{0, 2}, {3, 1}}
    return depth == H264MI_DEPTH_TRUNC ? 0u : 0x00020002u;
}
PICDEV uint32_t deep_add_at(uint32_t add, int x) { return (x & 1) ? add >> 16 : add & 0xffffu; }
PICDEV uint32_t deep_narrow1(uint32_t v10, uint32_t add) { return min(255u, (v10 + add) >> 2); }

// the 10-bit values of a dword's two words
template <bool MSB>
PICDEV deep_pk deep_val2(uint32_t x) { return MSB ? deep_as_pk(x) >> (unsigned short)6 : deep_as_pk(x) & (unsigned short)1023; }
// two 10-bit values to two 8-bit ones, in place in their fields
PICDEV uint32_t deep_narrow2(deep_pk v, uint32_t add) {
    const deep_pk t = (v + deep_as_pk(add)) >> (unsigned short)2;
    return deep_as_u32(__builtin_elementwise_min(t, (deep_pk)(unsigned short)255));
}
// (a + b + 1) >> 1 of two pairs of 10-bit values
PICDEV deep_pk deep_avg2(deep_pk a, deep_pk b) { return (a + b + (unsigned short)1) >> (unsigned short)1; }
// bytes 0, 1 (LO) or 2, 3 (HI) of x as two words of a deep format
template <bool MSB, bool HI>
PICDEV uint32_t deep_widen2(uint32_t x) {
    if (MSB) return __builtin_amdgcn_perm(0u, x, HI ? DEEP_SEL_HIGH_HI : DEEP_SEL_HIGH_LO);
    return __builtin_amdgcn_perm(0u, x, HI ? PIX_SEL_WIDE_HI : PIX_SEL_WIDE_LO) << 2;
}
template <bool MSB>
PICDEV uint32_t deep_val1(uint16_t x) { return MSB ? x >> 6 : x & 1023; }
template <bool MSB>
PICDEV uint16_t deep_word1(uint32_t v8) { return (uint16_t)(MSB ? v8 << 8 : v8 << 2); }

// nb bytes of value 128 at d (Y800's chroma)
PICDEV void deep_fill_row(uint8_t *d, int nb, int lane) {
    const bool wide = pix_al(d, d, 15);
    for (int x = 16 * lane; x < nb; x += 16 * 64) {
        if (wide && x + 16 <= nb) *(uint4 *)(d + x) = make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
        else for (int j = 0; j < 16 && x + j < nb; j++) d[x + j] = 128;
    }
}

// I422 chroma: the 8-bit rows a, b (rows 2r, 2r + 1, n bytes) from (PACK) or to the I420 row c
template <bool PACK>
PICDEV void deep_422_rows(uint8_t *a, uint8_t *b, uint8_t *c, int n, int lane) {
    const bool wide = pix_al(a, b, 15) && pix_al(c, c, 15);
    for (int x = 16 * lane; x < n; x += 16 * 64) {
        if (wide && x + 16 <= n) {
            if (PACK) {
                const uint4 s = *(const uint4 *)(c + x);
                *(uint4 *)(a + x) = s;
                *(uint4 *)(b + x) = s;
            } else {
                const uint4 s = *(const uint4 *)(a + x), t = *(const uint4 *)(b + x);
                *(uint4 *)(c + x) = make_uint4(pix_avg4(s.x, t.x), pix_avg4(s.y, t.y), pix_avg4(s.z, t.z), pix_avg4(s.w, t.w));
            }
        } else {
            for (int j = 0; j < 16 && x + j < n; j++) {
                if (PACK) a[x + j] = b[x + j] = c[x + j];
                else c[x + j] = (uint8_t)((a[x + j] + b[x + j] + 1) >> 1);
            }
        }
    }
}

// the sum of the four samples of each 2x2 of two dwords of two rows, + 2, >> 2: two bytes in two 16-bit fields
PICDEV uint32_t deep_box2(uint32_t s, uint32_t t) {
    const deep_pk m = (deep_pk)(unsigned short)0x00ff;
    const deep_pk sum = (deep_as_pk(s) & m) + (deep_as_pk(s) >> (unsigned short)8) + (deep_as_pk(t) & m) + (deep_as_pk(t) >> (unsigned short)8);
    return deep_as_u32((sum + (unsigned short)2) >> (unsigned short)2);
}
// I444 chroma: the 8-bit rows a, b (2n bytes each) from (PACK) or to the I420 row c (n bytes)
template <bool PACK>
PICDEV void deep_444_rows(uint8_t *a, uint8_t *b, uint8_t *c, int n, int lane) {
    const bool wide = pix_al(a, b, 15) && pix_al(c, c, 7);
    for (int x = 8 * lane; x < n; x += 8 * 64) {
        if (wide && x + 8 <= n) {
            if (PACK) {
                const uint2 s = *(const uint2 *)(c + x);
                const uint4 o = make_uint4(__builtin_amdgcn_perm(s.x, s.x, PIX_SEL_ZIP_LO), __builtin_amdgcn_perm(s.x, s.x, PIX_SEL_ZIP_HI),
                                           __builtin_amdgcn_perm(s.y, s.y, PIX_SEL_ZIP_LO), __builtin_amdgcn_perm(s.y, s.y, PIX_SEL_ZIP_HI));
                *(uint4 *)(a + 2 * x) = o;
                *(uint4 *)(b + 2 * x) = o;
            } else {
                const uint4 s = *(const uint4 *)(a + 2 * x), t = *(const uint4 *)(b + 2 * x);  // both rows before the average
                uint2 o;
                o.x = __builtin_amdgcn_perm(deep_box2(s.y, t.y), deep_box2(s.x, t.x), PIX_SEL_EVEN);
                o.y = __builtin_amdgcn_perm(deep_box2(s.w, t.w), deep_box2(s.z, t.z), PIX_SEL_EVEN);
                *(uint2 *)(c + x) = o;
            }
        } else {
            for (int j = 0; j < 8 && x + j < n; j++) {
                const int k = x + j;
                if (PACK) a[2 * k] = a[2 * k + 1] = b[2 * k] = b[2 * k + 1] = c[k];
                else c[k] = (uint8_t)((a[2 * k] + a[2 * k + 1] + b[2 * k] + b[2 * k + 1] + 2) >> 2);
            }
        }
    }
}

// NV16 chroma: the interleaved 8-bit rows a, b (cw Cb Cr pairs each) from (PACK) or to the I420 rows u, v
template <bool PACK>
PICDEV void deep_nv16_rows(uint8_t *a, uint8_t *b, uint8_t *u, uint8_t *v, int cw, int lane) {
    const bool wide = pix_al(a, b, 15) && pix_al(u, v, 7);
    for (int c = 8 * lane; c < cw; c += 8 * 64) {
        if (wide && c + 8 <= cw) {
            if (PACK) {
                const uint2 cu = *(const uint2 *)(u + c), cv = *(const uint2 *)(v + c);
                const uint4 o = make_uint4(__builtin_amdgcn_perm(cv.x, cu.x, PIX_SEL_ZIP_LO), __builtin_amdgcn_perm(cv.x, cu.x, PIX_SEL_ZIP_HI),
                                           __builtin_amdgcn_perm(cv.y, cu.y, PIX_SEL_ZIP_LO), __builtin_amdgcn_perm(cv.y, cu.y, PIX_SEL_ZIP_HI));
                *(uint4 *)(a + 2 * c) = o;
                *(uint4 *)(b + 2 * c) = o;
            } else {
                const uint4 s = *(const uint4 *)(a + 2 * c), t = *(const uint4 *)(b + 2 * c);
                const uint32_t m0 = pix_avg4(s.x, t.x), m1 = pix_avg4(s.y, t.y), m2 = pix_avg4(s.z, t.z), m3 = pix_avg4(s.w, t.w);
                *(uint2 *)(u + c) = make_uint2(__builtin_amdgcn_perm(m1, m0, PIX_SEL_EVEN), __builtin_amdgcn_perm(m3, m2, PIX_SEL_EVEN));
                *(uint2 *)(v + c) = make_uint2(__builtin_amdgcn_perm(m1, m0, PIX_SEL_ODD), __builtin_amdgcn_perm(m3, m2, PIX_SEL_ODD));
            }
        } else {
            for (int j = 0; j < 8 && c + j < cw; j++) {
                const int k = c + j;
                if (PACK) { a[2 * k] = b[2 * k] = u[k]; a[2 * k + 1] = b[2 * k + 1] = v[k]; }
                else { u[k] = (uint8_t)((a[2 * k] + b[2 * k] + 1) >> 1); v[k] = (uint8_t)((a[2 * k + 1] + b[2 * k + 1] + 1) >> 1); }
            }
        }
    }
}

// planar 16-bit rows: n words at a, and at b when there are two (4:2:2 chroma rows 2r, 2r + 1; nullptr otherwise), from
// (PACK) or to the n bytes at c; add is deep_addend of c's row
template <bool PACK, bool MSB>
PICDEV void deep_planar_rows(uint8_t *a, uint8_t *b, uint8_t *c, int n, uint32_t add, int lane) {
    const bool wide = pix_al(a, b, 15) && pix_al(c, c, 7);  // a null b adds nothing
    for (int x = 8 * lane; x < n; x += 8 * 64) {
        if (wide && x + 8 <= n) {
            if (PACK) {
                const uint2 s = *(const uint2 *)(c + x);
                const uint4 o = make_uint4(deep_widen2<MSB, false>(s.x), deep_widen2<MSB, true>(s.x), deep_widen2<MSB, false>(s.y),
                                           deep_widen2<MSB, true>(s.y));
                *(uint4 *)(a + 2 * x) = o;
                if (b) *(uint4 *)(b + 2 * x) = o;
            } else {
                const uint4 s = *(const uint4 *)(a + 2 * x);
                deep_pk v0 = deep_val2<MSB>(s.x), v1 = deep_val2<MSB>(s.y), v2 = deep_val2<MSB>(s.z), v3 = deep_val2<MSB>(s.w);
                if (b) {
                    const uint4 t = *(const uint4 *)(b + 2 * x);
                    v0 = deep_avg2(v0, deep_val2<MSB>(t.x)); v1 = deep_avg2(v1, deep_val2<MSB>(t.y));
                    v2 = deep_avg2(v2, deep_val2<MSB>(t.z)); v3 = deep_avg2(v3, deep_val2<MSB>(t.w));
                }
                uint2 o;
                o.x = __builtin_amdgcn_perm(deep_narrow2(v1, add), deep_narrow2(v0, add), PIX_SEL_EVEN);
                o.y = __builtin_amdgcn_perm(deep_narrow2(v3, add), deep_narrow2(v2, add), PIX_SEL_EVEN);
                *(uint2 *)(c + x) = o;
            }
        } else {
            uint16_t *wa = (uint16_t *)a, *wb = (uint16_t *)b;
            for (int j = 0; j < 8 && x + j < n; j++) {
                const int k = x + j;
                if (PACK) {
                    wa[k] = deep_word1<MSB>(c[k]);
                    if (b) wb[k] = wa[k];
                } else {
                    uint32_t v = deep_val1<MSB>(wa[k]);
                    if (b) v = (v + deep_val1<MSB>(wb[k]) + 1) >> 1;
                    c[k] = (uint8_t)deep_narrow1(v, deep_add_at(add, k));
                }
            }
        }
    }
}

// interleaved 16-bit rows: cw Cb Cr word pairs at a, and at b when there are two (nullptr otherwise), from (PACK) or to
// the cw bytes each at u and v; add is deep_addend of the chroma row
template <bool PACK, bool MSB>
PICDEV void deep_il_rows(uint8_t *a, uint8_t *b, uint8_t *u, uint8_t *v, int cw, uint32_t add, int lane) {
    const bool wide = pix_al(a, b, 15) && pix_al(u, v, 3);
    const uint32_t add_e = (add & 0xffffu) * 0x00010001u, add_o = (add >> 16) * 0x00010001u;  // a dword is one position
    for (int c = 4 * lane; c < cw; c += 4 * 64) {
        if (wide && c + 4 <= cw) {
            if (PACK) {
                const uint32_t cu = *(const uint32_t *)(u + c), cv = *(const uint32_t *)(v + c);
                const uint32_t uv0 = __builtin_amdgcn_perm(cv, cu, PIX_SEL_ZIP_LO), uv1 = __builtin_amdgcn_perm(cv, cu, PIX_SEL_ZIP_HI);
                const uint4 o = make_uint4(deep_widen2<MSB, false>(uv0), deep_widen2<MSB, true>(uv0), deep_widen2<MSB, false>(uv1),
                                           deep_widen2<MSB, true>(uv1));
                *(uint4 *)(a + 4 * c) = o;
                if (b) *(uint4 *)(b + 4 * c) = o;
            } else {
                const uint4 s = *(const uint4 *)(a + 4 * c);
                deep_pk v0 = deep_val2<MSB>(s.x), v1 = deep_val2<MSB>(s.y), v2 = deep_val2<MSB>(s.z), v3 = deep_val2<MSB>(s.w);
                if (b) {
                    const uint4 t = *(const uint4 *)(b + 4 * c);
                    v0 = deep_avg2(v0, deep_val2<MSB>(t.x)); v1 = deep_avg2(v1, deep_val2<MSB>(t.y));
                    v2 = deep_avg2(v2, deep_val2<MSB>(t.z)); v3 = deep_avg2(v3, deep_val2<MSB>(t.w));
                }
                // Cb Cr Cb Cr of positions c, c + 1 and of c + 2, c + 3, then the split
                const uint32_t p01 = __builtin_amdgcn_perm(deep_narrow2(v1, add_o), deep_narrow2(v0, add_e), PIX_SEL_EVEN);
                const uint32_t p23 = __builtin_amdgcn_perm(deep_narrow2(v3, add_o), deep_narrow2(v2, add_e), PIX_SEL_EVEN);
                *(uint32_t *)(u + c) = __builtin_amdgcn_perm(p23, p01, PIX_SEL_EVEN);
                *(uint32_t *)(v + c) = __builtin_amdgcn_perm(p23, p01, PIX_SEL_ODD);
            }
        } else {
            uint16_t *wa = (uint16_t *)a, *wb = (uint16_t *)b;
            for (int j = 0; j < 4 && c + j < cw; j++) {
                const int k = c + j;
                if (PACK) {
                    wa[2 * k] = deep_word1<MSB>(u[k]); wa[2 * k + 1] = deep_word1<MSB>(v[k]);
                    if (b) { wb[2 * k] = wa[2 * k]; wb[2 * k + 1] = wa[2 * k + 1]; }
                } else {
                    uint32_t cu = deep_val1<MSB>(wa[2 * k]), cv = deep_val1<MSB>(wa[2 * k + 1]);
                    if (b) { cu = (cu + deep_val1<MSB>(wb[2 * k]) + 1) >> 1; cv = (cv + deep_val1<MSB>(wb[2 * k + 1]) + 1) >> 1; }
                    u[k] = (uint8_t)deep_narrow1(cu, deep_add_at(add, k));
                    v[k] = (uint8_t)deep_narrow1(cv, deep_add_at(add, k));
                }
            }
        }
    }
}

// ---- V210. A group's twelve fields in order are Cb0 Y0 Cr0 Y1 Cb1 Y2 Cr1 Y3 Cb2 Y4 Cr2 Y5: field f is bits
// 10 (f % 3) .. + 9 of word f / 3; Yk is field 2k + 1, Cbk field 4k, Crk field 4k + 2
PICDEV uint32_t v210_get(const uint32_t *wd, int f) { return (wd[f / 3] >> (10 * (f % 3))) & 1023u; }
// the words a, b of one group of rows 2r, 2r + 1 to six luma samples a row and three averaged Cb, Cr; gpar: the parity
// of the group's index in its row (its first chroma position is 3 * index)
PICDEV void v210_unpack_group(const uint32_t *a, const uint32_t *b, uint32_t *s0, uint32_t *s1, uint32_t *cu, uint32_t *cv, uint32_t add0,
                            uint32_t add1, uint32_t addc, int gpar) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
        s0[k] = deep_narrow1(v210_get(a, 2 * k + 1), deep_add_at(add0, k));
        s1[k] = deep_narrow1(v210_get(b, 2 * k + 1), deep_add_at(add1, k));
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t ad = deep_add_at(addc, gpar + k);
        cu[k] = deep_narrow1((v210_get(a, 4 * k) + v210_get(b, 4 * k) + 1) >> 1, ad);
        cv[k] = deep_narrow1((v210_get(a, 4 * k + 2) + v210_get(b, 4 * k + 2) + 1) >> 1, ad);
    }
}
// the other way: v << 2 in each field, bits 31..30 zero; a sample that is 0 leaves its field 0
PICDEV void v210_pack_group(uint32_t *a, uint32_t *b, const uint32_t *s0, const uint32_t *s1, const uint32_t *cu, const uint32_t *cv) {
#pragma unroll
    for (int k = 0; k < 4; k++) a[k] = b[k] = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const int f = 2 * k + 1;
        a[f / 3] |= s0[k] << (10 * (f % 3) + 2);
        b[f / 3] |= s1[k] << (10 * (f % 3) + 2);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int f = 4 * k, g = 4 * k + 2;
        const uint32_t x = cu[k] << (10 * (f % 3) + 2), y = cv[k] << (10 * (g % 3) + 2);
        a[f / 3] |= x; b[f / 3] |= x;
        a[g / 3] |= y; b[g / 3] |= y;
    }
}

// the V210 rows q0, q1 of a row pair from (PACK) or to the luma rows y0, y1 and the chroma rows u, v
template <bool PACK>
PICDEV void v210_row_pair(uint8_t *q0, uint8_t *q1, uint8_t *y0, uint8_t *y1, uint8_t *u, uint8_t *v, int w, int r, int depth, int lane) {
    const uint32_t add0 = deep_addend(depth, 2 * r), add1 = deep_addend(depth, 2 * r + 1), addc = deep_addend(depth, r);
    const bool wide = pix_al(q0, q1, 15) && pix_al(y0, y1, 15) && pix_al(u, v, 7);
    const int ngroups = (w + 5) / 6, nruns = wide ? w / 48 : 0;  // a run: eight whole groups
    for (int j = lane; j < nruns; j += 64) {
        uint8_t *pa = q0 + 128 * (size_t)j, *pb = q1 + 128 * (size_t)j;
        uint32_t ya[12], yb[12], cu[6], cv[6];
        if (PACK) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const uint4 s = *(const uint4 *)(y0 + 48 * j + 16 * k), t = *(const uint4 *)(y1 + 48 * j + 16 * k);
                ya[4 * k] = s.x; ya[4 * k + 1] = s.y; ya[4 * k + 2] = s.z; ya[4 * k + 3] = s.w;
                yb[4 * k] = t.x; yb[4 * k + 1] = t.y; yb[4 * k + 2] = t.z; yb[4 * k + 3] = t.w;
                const uint2 c = *(const uint2 *)(u + 24 * j + 8 * k), d = *(const uint2 *)(v + 24 * j + 8 * k);
                cu[2 * k] = c.x; cu[2 * k + 1] = c.y; cv[2 * k] = d.x; cv[2 * k + 1] = d.y;
            }
#pragma unroll
            for (int g = 0; g < 8; g++) {
                uint32_t s0[6], s1[6], c0[3], c1[3], a[4], b[4];
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    const int i = 6 * g + k;
                    s0[k] = (ya[i >> 2] >> (8 * (i & 3))) & 255u;
                    s1[k] = (yb[i >> 2] >> (8 * (i & 3))) & 255u;
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const int i = 3 * g + k;
                    c0[k] = (cu[i >> 2] >> (8 * (i & 3))) & 255u;
                    c1[k] = (cv[i >> 2] >> (8 * (i & 3))) & 255u;
                }
                v210_pack_group(a, b, s0, s1, c0, c1);
                *(uint4 *)(pa + 16 * g) = make_uint4(a[0], a[1], a[2], a[3]);
                *(uint4 *)(pb + 16 * g) = make_uint4(b[0], b[1], b[2], b[3]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 12; k++) ya[k] = yb[k] = 0;
#pragma unroll
            for (int k = 0; k < 6; k++) cu[k] = cv[k] = 0;
#pragma unroll
            for (int g = 0; g < 8; g++) {
                const uint4 s = *(const uint4 *)(pa + 16 * g), t = *(const uint4 *)(pb + 16 * g);
                const uint32_t a[4] = {s.x, s.y, s.z, s.w}, b[4] = {t.x, t.y, t.z, t.w};
                uint32_t s0[6], s1[6], c0[3], c1[3];
                v210_unpack_group(a, b, s0, s1, c0, c1, add0, add1, addc, g & 1);  // a run starts at an even group
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    const int i = 6 * g + k;
                    ya[i >> 2] |= s0[k] << (8 * (i & 3));
                    yb[i >> 2] |= s1[k] << (8 * (i & 3));
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const int i = 3 * g + k;
                    cu[i >> 2] |= c0[k] << (8 * (i & 3));
                    cv[i >> 2] |= c1[k] << (8 * (i & 3));
                }
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                *(uint4 *)(y0 + 48 * j + 16 * k) = make_uint4(ya[4 * k], ya[4 * k + 1], ya[4 * k + 2], ya[4 * k + 3]);
                *(uint4 *)(y1 + 48 * j + 16 * k) = make_uint4(yb[4 * k], yb[4 * k + 1], yb[4 * k + 2], yb[4 * k + 3]);
                *(uint2 *)(u + 24 * j + 8 * k) = make_uint2(cu[2 * k], cu[2 * k + 1]);
                *(uint2 *)(v + 24 * j + 8 * k) = make_uint2(cv[2 * k], cv[2 * k + 1]);
            }
        }
    }
    // one group a lane: the groups after the last run, the partial last group, and every group of an unaligned row pair
    for (int g = 8 * nruns + lane; g < ngroups; g += 64) {
        uint32_t *pa = (uint32_t *)(q0 + 16 * (size_t)g), *pb = (uint32_t *)(q1 + 16 * (size_t)g);
        const int x0 = 6 * g, c0i = 3 * g, ny = min(6, w - x0), nc = ny / 2;  // samples of the group inside the row
        uint32_t s0[6], s1[6], c0[3], c1[3], a[4], b[4];
        if (PACK) {
#pragma unroll
            for (int k = 0; k < 6; k++) { s0[k] = k < ny ? y0[x0 + k] : 0u; s1[k] = k < ny ? y1[x0 + k] : 0u; }
#pragma unroll
            for (int k = 0; k < 3; k++) { c0[k] = k < nc ? u[c0i + k] : 0u; c1[k] = k < nc ? v[c0i + k] : 0u; }
            v210_pack_group(a, b, s0, s1, c0, c1);
#pragma unroll
            for (int k = 0; k < 4; k++) { pa[k] = a[k]; pb[k] = b[k]; }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) { a[k] = pa[k]; b[k] = pb[k]; }
            v210_unpack_group(a, b, s0, s1, c0, c1, add0, add1, addc, g & 1);
#pragma unroll
            for (int k = 0; k < 6; k++)
                if (k < ny) { y0[x0 + k] = (uint8_t)s0[k]; y1[x0 + k] = (uint8_t)s1[k]; }
#pragma unroll
            for (int k = 0; k < 3; k++)
                if (k < nc) { u[c0i + k] = (uint8_t)c0[k]; v[c0i + k] = (uint8_t)c1[k]; }
        }
    }
}

// luma of the deep planar and semi-planar formats: rows 2r and 2r + 1, one row each call
template <bool PACK, bool MSB>
PICDEV void deep_luma(const PixFrame &f, int r, uint8_t *y0, int lane) {
    uint8_t *l0 = f.p[0] + (size_t)(2 * r) * f.pp[0];
    deep_planar_rows<PACK, MSB>(l0, nullptr, y0, f.w, deep_addend(f.depth, 2 * r), lane);
    deep_planar_rows<PACK, MSB>(l0 + f.pp[0], nullptr, y0 + f.ys, f.w, deep_addend(f.depth, 2 * r + 1), lane);
}

// row pair r (luma rows 2r, 2r + 1, I420 chroma row r) of a frame, one wave
template <bool PACK>
PICDEV void deep_row_pair(const PixFrame &f, int r, int lane) {
    uint8_t *y0 = f.y + (size_t)(2 * r) * f.ys, *u = f.u + (size_t)r * f.cs, *v = f.v + (size_t)r * f.cs;
    const int cw = f.w / 2;
    const uint32_t addc = deep_addend(f.depth, r);
    uint8_t *l0 = f.p[0] + (size_t)(2 * r) * f.pp[0];
    switch (f.pix) {
    case H264MI_PIX_V210:
        v210_row_pair<PACK>(l0, l0 + f.pp[0], y0, y0 + f.ys, u, v, f.w, r, f.depth, lane);
        return;
    case H264MI_PIX_P010: case H264MI_PIX_P210: {
        deep_luma<PACK, true>(f, r, y0, lane);
        const bool two = f.pix == H264MI_PIX_P210;
        uint8_t *c0 = f.p[1] + (size_t)(two ? 2 * r : r) * f.pp[1];
        deep_il_rows<PACK, true>(c0, two ? c0 + f.pp[1] : nullptr, u, v, cw, addc, lane);
        return;
    }
    case H264MI_PIX_I010: case H264MI_PIX_I210: {
        deep_luma<PACK, false>(f, r, y0, lane);
        const bool two = f.pix == H264MI_PIX_I210;
        uint8_t *a = f.p[1] + (size_t)(two ? 2 * r : r) * f.pp[1], *b = f.p[2] + (size_t)(two ? 2 * r : r) * f.pp[2];
        deep_planar_rows<PACK, false>(a, two ? a + f.pp[1] : nullptr, u, cw, addc, lane);
        deep_planar_rows<PACK, false>(b, two ? b + f.pp[2] : nullptr, v, cw, addc, lane);
        return;
    }
    default: break;
    }
    if (PACK) pix_move_rows(l0, f.pp[0], y0, f.ys, f.w, 2, lane);
    else pix_move_rows(y0, f.ys, l0, f.pp[0], f.w, 2, lane);
    if (f.pix == H264MI_PIX_Y800) {
        if (!PACK) { deep_fill_row(u, cw, lane); deep_fill_row(v, cw, lane); }
        return;
    }
    uint8_t *a = f.p[1] + (size_t)(2 * r) * f.pp[1];
    if (f.pix == H264MI_PIX_NV16) {
        deep_nv16_rows<PACK>(a, a + f.pp[1], u, v, cw, lane);
        return;
    }
    uint8_t *b = f.p[2] + (size_t)(2 * r) * f.pp[2];
    if (f.pix == H264MI_PIX_I422) {
        deep_422_rows<PACK>(a, a + f.pp[1], u, cw, lane);
        deep_422_rows<PACK>(b, b + f.pp[2], v, cw, lane);
    } else {  // I444
        deep_444_rows<PACK>(a, a + f.pp[1], u, cw, lane);
        deep_444_rows<PACK>(b, b + f.pp[2], v, cw, lane);
    }
}

// ---- host
int launch_pixdeep_to_i420(uint8_t *d_i420, const uint8_t *d_src, const h264mi_pix_layout &L, int depth, int w, int h, int n, hipStream_t s) {
    return launch_pix_rows<deep_row_pair<false>>(d_src, L, d_i420, depth, w, h, n, s);
}
int launch_i420_to_pixdeep(uint8_t *d_dst, const h264mi_pix_layout &L, const uint8_t *d_i420, int w, int h, int n, hipStream_t s) {
    return launch_pix_rows<deep_row_pair<true>>(d_dst, L, d_i420, 0, w, h, n, s);
}
int launch_dec_output_pixdeep(int S, int cw, int ch, int w, int h, const DecDesc *desc, const DecInput *in, const h264mi_pix_layout &L,
                              hipStream_t s) {
    return launch_dec_output_rows<deep_row_pair<true>>(S, cw, ch, w, h, desc, in, L, s);
}
}  // namespace h264mi
