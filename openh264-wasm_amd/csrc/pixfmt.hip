// pixfmt.hip -- frames in other memory layouts to and from tight I420 on the device (gfx950): NV12, NV21, YUY2, UYVY
// and I420 with pitches, as include/h264mi.h (h264mi_pix_layout) defines them. DESIGN.md §5.10.
//   pix_rows_kernel<pix_row_pair<false>>       : n frames in a layout -> n tight I420 frames (h264mi_pix_to_i420_dev,
//                                                h264mi_enc_encode_pix)
//   pix_rows_kernel<pix_row_pair<true>>        : n tight I420 frames -> n frames in a layout (h264mi_i420_to_pix_dev)
//   dec_output_rows_kernel<pix_row_pair<true>> : the batch decoder's per-frame read-out into a layout
//                           (h264mi_dec_set_output_layout): the cropped picture read where it lies (coded strides, crop
//                           origin), as dec_output_rgba_kernel
// The kernels, their launchers, the frame and the plain row move are pix_rows.h's, shared with pixdeep.hip; this file
// owns the row functions of its five formats. One definition for all three kernels (pix_row_pair): the "layout side" of a frame is up to three planes with a pitch each,
// the "I420 side" three plane pointers with a luma and a chroma pitch (tight for the conversions, the coded strides for
// the decoder). Samples are moved; the one computed value is the 4:2:2 -> 4:2:0 chroma, (a + b + 1) >> 1 of rows 2y, 2y+1.
//
// Work split. The unit is a row pair: luma rows 2r and 2r + 1 and chroma row r, which is what one row of interleaved
// or planar chroma, and two rows of packed 4:2:2, belong to. A wave owns one row pair of one frame, a block of four
// waves a strip of four row pairs; blocks stride over (frame, strip), at most PIC_MAX_BLOCKS of them. Inside a row the
// 64 lanes take consecutive pieces and loop when the row is longer than the wave's reach (1024 bytes of the widest side).
//
// Access widths, why. These are streaming kernels: every byte is read once and written once, so the cost is the number
// of memory instructions and whether a wave's instruction covers whole consecutive lines. 16 bytes a lane is the widest
// vector access (global_load/store_dwordx4): 64 lanes x 16 B = 1 KiB per instruction, the form the HBM-bound rate is
// quoted for, and a quarter of the instructions of dword accesses. The side with the most bytes per sample sets the
// piece a lane owns, so that this side moves as dwordx4 and the others as the widest access that holds the same samples:
//   planar rows (Y of every format but the packed ones; Cb, Cr of pitched I420): 16 bytes in, 16 bytes out, both rows
//     of the pair loaded before either is stored
//   NV12 / NV21 chroma row: 16 interleaved bytes = 8 Cb + 8 Cr: one dwordx4 on the interleaved side, two dwordx2 on the
//     planar side. (de)interleaved in registers with four v_perm_b32
//   YUY2 / UYVY row pair: 16 packed bytes a row = 8 Y + 4 Cb + 4 Cr: one dwordx4 per row on the packed side, one
//     dwordx2 of luma per row and one dword each of Cb and Cr per row pair on the planar side. Twelve v_perm_b32
//     interleave a pair of rows (the chroma pair is built once for both rows); the other way eight de-interleave them
//     and the average runs on packed bytes: each dword of Cb Cr pairs widened to two dwords of 16-bit fields (v_perm_b32
//     with the zero selector), added with the rounding 1 in each field, shifted, and narrowed again by one v_perm_b32.
//   The planar accesses of a lane are narrower there (8 and 4 bytes), but consecutive lanes still cover consecutive
//   bytes, 512 and 256 per instruction, whole 128-byte lines each.
// Two paths for the same bytes, chosen per plane (per row-pair operation) and frame from the pointers of the rows it
// touches: when every one of them is a multiple of its access width the pieces that lie wholly inside the row take the
// wide path; a piece that crosses the row's end, and every piece of a row whose pointers are not aligned (a buffer at
// an odd address, a pitch that is no multiple of 16, w % 16 != 0), takes bytes -- the same values by the same rule.
// An aligned piece that ends inside the row never leaves it, and the byte path stops at the row's end: no access leaves
// the rows the layout names, on either side, and pitch padding and gaps are never written.
//
// A translation unit and a code object of its own, as orient.hip is. The host runtime (capi_enc.inc, runtime_dec.inc) reaches it through the functions picture_host.h
// declares; the layout rules are host code there (pix_span, pix_layout_ok).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include "../../include/h264mi.h"
#include "pix_rows.h"

namespace h264mi {
// one interleaved chroma row il (cw pairs: a[i] at byte 2i, b[i] at 2i + 1) from (PACK) or to the planar rows a, b
template <bool PACK>
PICDEV void pix_nv_row(uint8_t *il, uint8_t *a, uint8_t *b, int cw, int lane) {
    const bool wide = pix_al(il, il, 15) && pix_al(a, b, 7);
    for (int c = 8 * lane; c < cw; c += 8 * 64) {
        if (wide && c + 8 <= cw) {
            if (PACK) {
                const uint2 va = *(const uint2 *)(a + c), vb = *(const uint2 *)(b + c);
                uint4 o;
                o.x = __builtin_amdgcn_perm(vb.x, va.x, PIX_SEL_ZIP_LO);
                o.y = __builtin_amdgcn_perm(vb.x, va.x, PIX_SEL_ZIP_HI);
                o.z = __builtin_amdgcn_perm(vb.y, va.y, PIX_SEL_ZIP_LO);
                o.w = __builtin_amdgcn_perm(vb.y, va.y, PIX_SEL_ZIP_HI);
                *(uint4 *)(il + 2 * c) = o;
            } else {
                const uint4 i = *(const uint4 *)(il + 2 * c);
                uint2 va, vb;
                va.x = __builtin_amdgcn_perm(i.y, i.x, PIX_SEL_EVEN);
                vb.x = __builtin_amdgcn_perm(i.y, i.x, PIX_SEL_ODD);
                va.y = __builtin_amdgcn_perm(i.w, i.z, PIX_SEL_EVEN);
                vb.y = __builtin_amdgcn_perm(i.w, i.z, PIX_SEL_ODD);
                *(uint2 *)(a + c) = va;
                *(uint2 *)(b + c) = vb;
            }
        } else {
            for (int j = 0; j < 8 && c + j < cw; j++) {
                if (PACK) { il[2 * (c + j)] = a[c + j]; il[2 * (c + j) + 1] = b[c + j]; }
                else { a[c + j] = il[2 * (c + j)]; b[c + j] = il[2 * (c + j) + 1]; }
            }
        }
    }
}

// the packed rows q0, q1 (2w bytes each) of a row pair from (PACK) or to the luma rows y0, y1 and the chroma rows u, v.
// yo: 0 YUY2 (luma in the even bytes), 1 UYVY (in the odd ones)
template <bool PACK>
PICDEV void pix_422_row_pair(uint8_t *q0, uint8_t *q1, uint8_t *y0, uint8_t *y1, uint8_t *u, uint8_t *v, int w, int yo, int lane) {
    const bool wide = pix_al(q0, q1, 15) && pix_al(y0, y1, 7) && pix_al(u, v, 3);
    const uint32_t ysel = yo ? PIX_SEL_ODD : PIX_SEL_EVEN, csel = yo ? PIX_SEL_EVEN : PIX_SEL_ODD;
    for (int x = 8 * lane; x < w; x += 8 * 64) {
        if (wide && x + 8 <= w) {
            if (PACK) {
                const uint2 ya = *(const uint2 *)(y0 + x), yb = *(const uint2 *)(y1 + x);
                const uint32_t cu = *(const uint32_t *)(u + x / 2), cv = *(const uint32_t *)(v + x / 2);
                const uint32_t uv0 = __builtin_amdgcn_perm(cv, cu, PIX_SEL_ZIP_LO), uv1 = __builtin_amdgcn_perm(cv, cu, PIX_SEL_ZIP_HI);
                uint4 a, b;  // the bytes at even positions come from the second operand
                a.x = __builtin_amdgcn_perm(yo ? ya.x : uv0, yo ? uv0 : ya.x, PIX_SEL_ZIP_LO);
                a.y = __builtin_amdgcn_perm(yo ? ya.x : uv0, yo ? uv0 : ya.x, PIX_SEL_ZIP_HI);
                a.z = __builtin_amdgcn_perm(yo ? ya.y : uv1, yo ? uv1 : ya.y, PIX_SEL_ZIP_LO);
                a.w = __builtin_amdgcn_perm(yo ? ya.y : uv1, yo ? uv1 : ya.y, PIX_SEL_ZIP_HI);
                b.x = __builtin_amdgcn_perm(yo ? yb.x : uv0, yo ? uv0 : yb.x, PIX_SEL_ZIP_LO);
                b.y = __builtin_amdgcn_perm(yo ? yb.x : uv0, yo ? uv0 : yb.x, PIX_SEL_ZIP_HI);
                b.z = __builtin_amdgcn_perm(yo ? yb.y : uv1, yo ? uv1 : yb.y, PIX_SEL_ZIP_LO);
                b.w = __builtin_amdgcn_perm(yo ? yb.y : uv1, yo ? uv1 : yb.y, PIX_SEL_ZIP_HI);
                *(uint4 *)(q0 + 2 * x) = a;
                *(uint4 *)(q1 + 2 * x) = b;
            } else {
                const uint4 a = *(const uint4 *)(q0 + 2 * x), b = *(const uint4 *)(q1 + 2 * x);
                uint2 ya, yb;
                ya.x = __builtin_amdgcn_perm(a.y, a.x, ysel);
                ya.y = __builtin_amdgcn_perm(a.w, a.z, ysel);
                yb.x = __builtin_amdgcn_perm(b.y, b.x, ysel);
                yb.y = __builtin_amdgcn_perm(b.w, b.z, ysel);
                // Cb Cr pairs of each row, averaged while still interleaved, then split
                const uint32_t uv0 = pix_avg4(__builtin_amdgcn_perm(a.y, a.x, csel), __builtin_amdgcn_perm(b.y, b.x, csel));
                const uint32_t uv1 = pix_avg4(__builtin_amdgcn_perm(a.w, a.z, csel), __builtin_amdgcn_perm(b.w, b.z, csel));
                *(uint2 *)(y0 + x) = ya;
                *(uint2 *)(y1 + x) = yb;
                *(uint32_t *)(u + x / 2) = __builtin_amdgcn_perm(uv1, uv0, PIX_SEL_EVEN);
                *(uint32_t *)(v + x / 2) = __builtin_amdgcn_perm(uv1, uv0, PIX_SEL_ODD);
            }
        } else {
            for (int j = 0; j < 8 && x + j < w; j += 2) {  // w is even: a sample pair a step
                const int k = x + j, c = k / 2;
                uint8_t *a = q0 + 2 * k, *b = q1 + 2 * k;
                if (PACK) {
                    a[yo] = y0[k]; a[2 + yo] = y0[k + 1]; b[yo] = y1[k]; b[2 + yo] = y1[k + 1];
                    a[1 - yo] = b[1 - yo] = u[c];
                    a[3 - yo] = b[3 - yo] = v[c];
                } else {
                    y0[k] = a[yo]; y0[k + 1] = a[2 + yo]; y1[k] = b[yo]; y1[k + 1] = b[2 + yo];
                    u[c] = (uint8_t)((a[1 - yo] + b[1 - yo] + 1) >> 1);
                    v[c] = (uint8_t)((a[3 - yo] + b[3 - yo] + 1) >> 1);
                }
            }
        }
    }
}

// row pair r (luma rows 2r, 2r + 1, chroma row r) of a frame, one wave
template <bool PACK>
PICDEV void pix_row_pair(const PixFrame &f, int r, int lane) {
    uint8_t *y0 = f.y + (size_t)(2 * r) * f.ys, *u = f.u + (size_t)r * f.cs, *v = f.v + (size_t)r * f.cs;
    if (f.pix == H264MI_PIX_YUY2 || f.pix == H264MI_PIX_UYVY) {
        uint8_t *q0 = f.p[0] + (size_t)(2 * r) * f.pp[0];
        pix_422_row_pair<PACK>(q0, q0 + f.pp[0], y0, y0 + f.ys, u, v, f.w, f.pix == H264MI_PIX_UYVY, lane);
        return;
    }
    uint8_t *l0 = f.p[0] + (size_t)(2 * r) * f.pp[0];
    if (PACK) pix_move_rows(l0, f.pp[0], y0, f.ys, f.w, 2, lane);
    else pix_move_rows(y0, f.ys, l0, f.pp[0], f.w, 2, lane);
    if (f.pix == H264MI_PIX_I420) {
        uint8_t *pu = f.p[1] + (size_t)r * f.pp[1], *pv = f.p[2] + (size_t)r * f.pp[2];
        if (PACK) { pix_move_rows(pu, 0, u, 0, f.w / 2, 1, lane); pix_move_rows(pv, 0, v, 0, f.w / 2, 1, lane); }
        else { pix_move_rows(u, 0, pu, 0, f.w / 2, 1, lane); pix_move_rows(v, 0, pv, 0, f.w / 2, 1, lane); }
    } else {  // NV12: Cb first; NV21: Cr first
        uint8_t *il = f.p[1] + (size_t)r * f.pp[1];
        const bool cb_first = f.pix == H264MI_PIX_NV12;
        pix_nv_row<PACK>(il, cb_first ? u : v, cb_first ? v : u, f.w / 2, lane);
    }
}

// ---- host
int launch_pix_to_i420(uint8_t *d_i420, const uint8_t *d_src, const h264mi_pix_layout &L, int w, int h, int n, hipStream_t s) {
    return launch_pix_rows<pix_row_pair<false>>(d_src, L, d_i420, 0, w, h, n, s);
}
int launch_i420_to_pix(uint8_t *d_dst, const h264mi_pix_layout &L, const uint8_t *d_i420, int w, int h, int n, hipStream_t s) {
    return launch_pix_rows<pix_row_pair<true>>(d_dst, L, d_i420, 0, w, h, n, s);
}
int launch_dec_output_pix(int S, int cw, int ch, int w, int h, const DecDesc *desc, const DecInput *in, const h264mi_pix_layout &L,
                          hipStream_t s) {
    return launch_dec_output_rows<pix_row_pair<true>>(S, cw, ch, w, h, desc, in, L, s);
}
}  // namespace h264mi
