// colorspace.hip -- the RGBA edges of the batch API under a colour specification (gfx950): BT.601 or BT.709, limited or
// full range, chroma picked or averaged on the way in and repeated or interpolated on the way out, as include/h264mi.h
// (h264mi_colorspec) defines them. DESIGN.md §5.11.
//   rgba_to_i420_cs_kernel<AVG, ALPHA> : n tight RGBA frames -> n tight I420 frames (h264mi_rgba_to_i420_cs_dev,
//                                        h264mi_enc_encode_rgba under a specification) or, ALPHA, n I420A sprites
//                                        (h264mi_rgba_to_i420a_cs_dev)
//   i420_to_rgba_cs_kernel<BIL>        : n tight I420 frames -> n tight RGBA frames (h264mi_i420_to_rgba_cs_dev)
//   dec_output_rgba_cs_kernel<BIL>     : the batch decoder's H264MI_FMT_RGBA read-out under a specification: the cropped
//                                        picture read where it lies (coded strides, crop origin), as dec_output_rgba_kernel
// The matrix and the range are one row of the table in picture_host.h (cs_coef) and travel as kernel arguments, so they
// sit in scalar registers; the chroma mode is a template argument, so a kernel carries one mode's code only.
//
// Work split: color.inc's. A lane converts 8 adjacent pixels on 2 rows (a unit): two 16-byte RGBA accesses a row, one
// 8-byte Y access a row, one 4-byte access to Cb and to Cr. Lanes are consecutive units of the frame in raster order,
// blocks stride over a frame's units and blockIdx.y over the frames. A unit holds whole 2x2 blocks, so AVERAGE needs
// nothing from outside the lane. The wide form needs w % 8 == 0, a 16-byte aligned RGBA frame, 8-byte aligned Y (and A)
// rows and 4-byte aligned chroma rows, tested per frame; otherwise the unit's pixels move as 4-byte RGBA pixels and
// single plane bytes, and a unit that crosses the row's end stops there. Both paths run the same arithmetic on the same
// values (cs_in_unit / cs_out_unit; only the loads and stores differ), so they give the same bytes. No access
// leaves its frame.
//
// BILINEAR. A unit's 4 chroma columns need their two neighbours, on the chroma row itself and on the rows above and
// below: 6 columns on 3 rows of Cb and of Cr, every index clamped to the picture (for the decoder: the cropped picture).
// They come by plain loads -- a dword and two bytes a row and plane on the wide path -- and not through an LDS strip:
//   * the bytes are few and already near. Chroma is 0.5 of the 5.5 bytes a pixel moves; the two extra rows are the rows
//     the neighbouring row pairs load anyway, one block (or a few) away in the same launch, so they are served by the
//     L2 (4 MiB an XCD, 34 TB/s against HBM's 6.3) or the L1, and the side bytes share a 64-byte line with the dword of
//     the same lane or its neighbour. HBM traffic stays 5.5 w h.
//   * an LDS strip would make the block, not the lane, the unit of work: a barrier a strip, a halo of rows and columns
//     a block, and a second geometry for the decoder's coded strides, to save loads that do not reach memory. Nothing
//     is reused inside a block that the lane does not already hold in registers: the vertical sums 3 C[cy] + C[ny] of a
//     unit's 6 columns are formed once a row and serve its 8 pixels.
// The cost is instructions: 18 chroma loads a unit instead of 2, and an interpolation a pixel where REPEAT shares one
// chroma pair among four. tools/cs_ab.py measures it.
//
// Products are 24-bit (coefficients below 2^10, samples and sums of four below 2^10, IY (Y - yo) below 2^17), so every
// multiply is the full-rate v_mul_i32_i24 / v_mad_i32_i24 (__mul24): the coefficients are runtime values, and a plain
// 32-bit multiply by one is the quarter-rate v_mul_lo_u32.
//
// A translation unit and a code object of its own, as pixfmt.hip is: the library's other kernels stay byte for byte what
// they were. The runtime (capi_enc.inc, capi_dec.inc, runtime_dec.inc) reaches it through the functions picture_host.h
// declares; the default specification never comes here from an encoder or a decoder.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include "../../include/h264mi.h"
#include "h264mi_types.h"
#include "picture_host.h"
#include "picture_dev.h"

namespace h264mi {
#define H264MI_CS_MAX_FRAMES_Y 256  // frames on blockIdx.y; further frames are a stride loop

PICDEV int cs_clamp8(int v) { return min(max(v, 0), 255); }
PICDEV uint32_t cs_pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return a | (b << 8) | (c << 16) | (d << 24); }
PICDEV int cs_byte(uint32_t v, int k) { return (int)((v >> (8 * k)) & 255); }
PICDEV int cs_dot(const int32_t *f, int r, int g, int b) { return __mul24(f[0], r) + __mul24(f[1], g) + __mul24(f[2], b); }

// ---- RGBA -> 4:2:0
// One RGBA pixel (R | G << 8 | B << 16 | A << 24) to Y
PICDEV uint32_t cs_y(const CsCoef &k, uint32_t p) {
    return (uint32_t)cs_clamp8(((cs_dot(k.fy, cs_byte(p, 0), cs_byte(p, 1), cs_byte(p, 2)) + 128) >> 8) + k.yo);
}
// The 2x2 block p00 p01 / p10 p11 to Cb (f = k.fu) or Cr (k.fv): of p00, or of the sum of the four
template <bool AVG>
PICDEV uint32_t cs_c(const int32_t *f, uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11) {
    if (AVG) {
        const int r = cs_byte(p00, 0) + cs_byte(p01, 0) + cs_byte(p10, 0) + cs_byte(p11, 0);
        const int g = cs_byte(p00, 1) + cs_byte(p01, 1) + cs_byte(p10, 1) + cs_byte(p11, 1);
        const int b = cs_byte(p00, 2) + cs_byte(p01, 2) + cs_byte(p10, 2) + cs_byte(p11, 2);
        return (uint32_t)cs_clamp8(((cs_dot(f, r, g, b) + 512) >> 10) + 128);
    }
    return (uint32_t)cs_clamp8(((cs_dot(f, cs_byte(p00, 0), cs_byte(p00, 1), cs_byte(p00, 2)) + 128) >> 8) + 128);
}

// A unit's 8 x 2 pixels p[row][i] to its bytes: y[row][i], a[row][i] (ALPHA), cb[j] and cr[j] of the 2x2 block j
template <bool AVG, bool ALPHA>
PICDEV void cs_in_unit(const CsCoef &k, const uint32_t (&p)[2][8], uint32_t (&y)[2][8], uint32_t (&a)[2][8], uint32_t (&cb)[4], uint32_t (&cr)[4]) {
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int i = 0; i < 8; i++) {
            y[r][i] = cs_y(k, p[r][i]);
            if (ALPHA) a[r][i] = p[r][i] >> 24;
        }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        cb[j] = cs_c<AVG>(k.fu, p[0][2 * j], p[0][2 * j + 1], p[1][2 * j], p[1][2 * j + 1]);
        cr[j] = cs_c<AVG>(k.fv, p[0][2 * j], p[0][2 * j + 1], p[1][2 * j], p[1][2 * j + 1]);
    }
}

struct CsInLaunch { const uint8_t *rgba; uint8_t *out; int w, h, n; CsCoef k; };

// n tight RGBA frames -> n tight I420 frames (ALPHA: I420A sprites: Y, Cb, Cr, then A). Grid (blocks over a frame's
// units, frames), both capped
template <bool AVG, bool ALPHA>
__global__ __launch_bounds__(256) void rgba_to_i420_cs_kernel(CsInLaunch a) {
    const int w = a.w, h = a.h, cw = w >> 1, upr = (w + 7) >> 3, units = upr * (h >> 1);
    const size_t ysz = (size_t)w * h, csz = (size_t)cw * (h >> 1);
    const size_t fin = ysz * 4, fout = (ALPHA ? 2 : 1) * ysz + 2 * csz;
    for (int f = blockIdx.y; f < a.n; f += gridDim.y) {
        const uint8_t *src = a.rgba + (size_t)f * fin;
        uint8_t *Y = a.out + (size_t)f * fout, *U = Y + ysz, *V = U + csz, *A = V + csz;
        const bool vec = ((w & 7) | ((uintptr_t)src & 15) | ((uintptr_t)Y & 7) | ((uintptr_t)U & 3) | ((uintptr_t)V & 3) |
                          (ALPHA ? ((uintptr_t)A & 7) : 0)) == 0;
        for (int u = blockIdx.x * 256 + threadIdx.x; u < units; u += gridDim.x * 256) {
            const int by = u / upr, x = (u - by * upr) * 8;
            const uint8_t *s0 = src + ((size_t)(2 * by) * w + x) * 4, *s1 = s0 + (size_t)w * 4;
            const size_t yo = (size_t)(2 * by) * w + x, c = (size_t)by * cw + (x >> 1);
            const int np = min(8, w - x);  // pixels of the unit inside the row: 8 on the wide path, even everywhere
            uint32_t p[2][8], y[2][8], al[2][8], cb[4], cr[4];
            if (vec) {
                const uint4 a0 = *(const uint4 *)s0, a1 = *(const uint4 *)(s0 + 16), b0 = *(const uint4 *)s1, b1 = *(const uint4 *)(s1 + 16);
                p[0][0] = a0.x; p[0][1] = a0.y; p[0][2] = a0.z; p[0][3] = a0.w; p[0][4] = a1.x; p[0][5] = a1.y; p[0][6] = a1.z; p[0][7] = a1.w;
                p[1][0] = b0.x; p[1][1] = b0.y; p[1][2] = b0.z; p[1][3] = b0.w; p[1][4] = b1.x; p[1][5] = b1.y; p[1][6] = b1.z; p[1][7] = b1.w;
            } else {
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    p[0][i] = i < np ? ((const uint32_t *)s0)[i] : 0;
                    p[1][i] = i < np ? ((const uint32_t *)s1)[i] : 0;
                }
            }
            cs_in_unit<AVG, ALPHA>(a.k, p, y, al, cb, cr);
            if (vec) {
                *(uint2 *)(Y + yo) = make_uint2(cs_pack4(y[0][0], y[0][1], y[0][2], y[0][3]), cs_pack4(y[0][4], y[0][5], y[0][6], y[0][7]));
                *(uint2 *)(Y + yo + w) = make_uint2(cs_pack4(y[1][0], y[1][1], y[1][2], y[1][3]), cs_pack4(y[1][4], y[1][5], y[1][6], y[1][7]));
                *(uint32_t *)(U + c) = cs_pack4(cb[0], cb[1], cb[2], cb[3]);
                *(uint32_t *)(V + c) = cs_pack4(cr[0], cr[1], cr[2], cr[3]);
                if (ALPHA) {
                    *(uint2 *)(A + yo) = make_uint2(cs_pack4(al[0][0], al[0][1], al[0][2], al[0][3]), cs_pack4(al[0][4], al[0][5], al[0][6], al[0][7]));
                    *(uint2 *)(A + yo + w) = make_uint2(cs_pack4(al[1][0], al[1][1], al[1][2], al[1][3]), cs_pack4(al[1][4], al[1][5], al[1][6], al[1][7]));
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    if (i >= np) break;
                    Y[yo + i] = (uint8_t)y[0][i];
                    Y[yo + w + i] = (uint8_t)y[1][i];
                    if (ALPHA) { A[yo + i] = (uint8_t)al[0][i]; A[yo + w + i] = (uint8_t)al[1][i]; }
                    if (!(i & 1)) { U[c + (i >> 1)] = (uint8_t)cb[i >> 1]; V[c + (i >> 1)] = (uint8_t)cr[i >> 1]; }
                }
            }
        }
    }
}

// ---- 4:2:0 -> RGBA
// Saturate before the shift, as color.inc's sat_shr8 and for its reason: the shift-then-saturate form matches
// v_ashr_pk_u8_i32, whose untouched upper half hipcc then takes for zero (toolchain notes)
PICDEV uint32_t cs_sat_shr8(int x) { return (uint32_t)min(max(x, 0), 65535) >> 8; }
// One pixel from its samples Y, Cb, Cr (0..255). The header's c + RV cr + 128 with c = IY (Y - yo), cr = Cr - 128 is
// IY Y + RV Cr + (128 - IY yo - 128 RV): the same integer, with the constant part (k.kr, kg, kb: cs_out_coef) formed once
// on the scalar unit. Written chroma first, so that pixels which share a chroma pair (REPEAT) share those terms too
struct CsOut { int iy, rv, gu, gv, bu, kr, kg, kb; };
PICDEV CsOut cs_out_coef(const CsCoef &k) {
    const int c = 128 - k.iy * k.yo;
    return CsOut{k.iy, k.rv, k.gu, k.gv, k.bu, c - 128 * k.rv, c + 128 * (k.gu + k.gv), c - 128 * k.bu};
}
PICDEV uint32_t cs_px(const CsOut &k, int y, int cb, int cr) {
    const int tr = __mul24(k.rv, cr) + k.kr, tg = k.kg - __mul24(k.gu, cb) - __mul24(k.gv, cr), tb = __mul24(k.bu, cb) + k.kb;
    return cs_sat_shr8(__mul24(k.iy, y) + tr) | (cs_sat_shr8(__mul24(k.iy, y) + tg) << 8) | (cs_sat_shr8(__mul24(k.iy, y) + tb) << 16) |
           0xff000000u;
}

// The chroma of one plane for a unit's 8 x 2 pixels, o[row][i] (0..255), from the plane's samples around the unit:
// m[j], t[j], b[j] = columns c0 - 1 + j (clamped to the picture) of the chroma rows cy, cy - 1 and cy + 1 (clamped).
// REPEAT reads m[1..4] only
template <bool BIL>
PICDEV void cs_out_chroma(const int (&m)[6], const int (&t)[6], const int (&b)[6], int (&o)[2][8]) {
    if (!BIL) {
#pragma unroll
        for (int i = 0; i < 8; i++) o[0][i] = o[1][i] = m[1 + (i >> 1)];
        return;
    }
    int v0[6], v1[6];  // 3 C[cy] + C[ny] for the upper luma row (ny = cy - 1) and the lower (ny = cy + 1)
#pragma unroll
    for (int j = 0; j < 6; j++) { v0[j] = 3 * m[j] + t[j]; v1[j] = 3 * m[j] + b[j]; }
#pragma unroll
    for (int j = 1; j < 5; j++) {  // the two pixels of column j share 3 v[j] + 8
        const int w0 = 3 * v0[j] + 8, w1 = 3 * v1[j] + 8;
        o[0][2 * j - 2] = (w0 + v0[j - 1]) >> 4; o[0][2 * j - 1] = (w0 + v0[j + 1]) >> 4;
        o[1][2 * j - 2] = (w1 + v1[j - 1]) >> 4; o[1][2 * j - 1] = (w1 + v1[j + 1]) >> 4;
    }
    // No instruction: the values become opaque to the compiler. __mul24 is (x << 8 >> 8) * (y << 8 >> 8) in the device
    // library; LLVM's IR passes can bound these sums, drop the shifts and leave a plain multiply, for which instruction
    // selection, whose own bound analysis gives up at this depth, then takes the quarter-rate v_mul_lo_u32 (50 a unit).
    // Opaque operands keep the shifts, and the shifted form selects v_mad_i32_i24
#pragma unroll
    for (int i = 0; i < 8; i++) { asm("" : "+v"(o[0][i])); asm("" : "+v"(o[1][i])); }
}

// 6 samples of the chroma row at `row` (cw samples) around columns c0 .. c0 + 3: c0 - 1 + j clamped to 0 .. cw - 1
template <bool VEC>
PICDEV void cs_row6(const uint8_t *row, int c0, int cw, int (&o)[6]) {
    if (VEC) {  // c0 + 3 < cw and row + c0 is 4-byte aligned
        const uint32_t d = *(const uint32_t *)(row + c0);
        o[0] = row[max(c0 - 1, 0)];
        o[1] = cs_byte(d, 0); o[2] = cs_byte(d, 1); o[3] = cs_byte(d, 2); o[4] = cs_byte(d, 3);
        o[5] = row[min(c0 + 4, cw - 1)];
    } else {
#pragma unroll
        for (int j = 0; j < 6; j++) o[j] = row[min(max(c0 - 1 + j, 0), cw - 1)];
    }
}

// One picture's planes and its tight RGBA frame
struct CsPic { const uint8_t *Y, *U, *V; int ys, uvs, w, h; uint8_t *rgba; };

// Unit u of a picture. VEC: the wide accesses; else 4-byte RGBA pixels and plane bytes, ending at the row's end. The
// arithmetic between the loads and the stores is the same code on the same values
template <bool BIL, bool VEC>
PICDEV void cs_out_unit(const CsOut &k, const CsPic &p, int u) {
    const int cw = p.w >> 1, ch = p.h >> 1, upr = (p.w + 7) >> 3;
    const int by = u / upr, x = (u - by * upr) * 8, c0 = x >> 1;
    const int np = VEC ? 8 : min(8, p.w - x);
    // offsets in int, products in 24 bits: rows and strides are below 2^14, a plane below 2^27 samples, a frame below 2^28 bytes
    const uint8_t *y0 = p.Y + (__mul24(2 * by, p.ys) + x), *y1 = y0 + p.ys;
    uint32_t *d0 = (uint32_t *)p.rgba + (__mul24(2 * by, p.w) + x), *d1 = d0 + p.w;
    int um[6], ut[6], ub[6], vm[6], vt[6], vb[6];
    cs_row6<VEC>(p.U + __mul24(by, p.uvs), c0, cw, um);
    cs_row6<VEC>(p.V + __mul24(by, p.uvs), c0, cw, vm);
    if (BIL) {
        const int rt = __mul24(max(by - 1, 0), p.uvs), rb = __mul24(min(by + 1, ch - 1), p.uvs);
        cs_row6<VEC>(p.U + rt, c0, cw, ut); cs_row6<VEC>(p.U + rb, c0, cw, ub);
        cs_row6<VEC>(p.V + rt, c0, cw, vt); cs_row6<VEC>(p.V + rb, c0, cw, vb);
    }
    int cb[2][8], cr[2][8], yy[2][8];
    cs_out_chroma<BIL>(um, ut, ub, cb);
    cs_out_chroma<BIL>(vm, vt, vb, cr);
    if (VEC) {
        const uint2 a = *(const uint2 *)y0, b = *(const uint2 *)y1;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            yy[0][i] = cs_byte(a.x, i); yy[0][4 + i] = cs_byte(a.y, i);
            yy[1][i] = cs_byte(b.x, i); yy[1][4 + i] = cs_byte(b.y, i);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) { yy[0][i] = i < np ? y0[i] : 0; yy[1][i] = i < np ? y1[i] : 0; }
    }
    uint32_t o[2][8];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int i = 0; i < 8; i++) o[r][i] = cs_px(k, yy[r][i], cb[r][i], cr[r][i]);
    if (VEC) {
        *(uint4 *)d0 = make_uint4(o[0][0], o[0][1], o[0][2], o[0][3]);
        *(uint4 *)(d0 + 4) = make_uint4(o[0][4], o[0][5], o[0][6], o[0][7]);
        *(uint4 *)d1 = make_uint4(o[1][0], o[1][1], o[1][2], o[1][3]);
        *(uint4 *)(d1 + 4) = make_uint4(o[1][4], o[1][5], o[1][6], o[1][7]);
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (i >= np) break;
            d0[i] = o[0][i];
            d1[i] = o[1][i];
        }
    }
}

// One w x h picture (even w and h; planes with strides ys / uvs) to a tight RGBA frame: the units u0, u0 + ustep, ...
// of the picture. Shared by the batched kernel and the decoder's read-out. Chroma indices clamp to w/2 x h/2. The path
// is chosen once a picture, outside the loop: inside it the compiler would weave the two into one body
template <bool BIL>
PICDEV void i420_to_rgba_cs_picture(const CsOut &k, const uint8_t *__restrict__ Y, const uint8_t *__restrict__ U, const uint8_t *__restrict__ V,
                                  int ys, int uvs, int w, int h, uint8_t *__restrict__ rgba, int u0, int ustep) {
    const int units = ((w + 7) >> 3) * (h >> 1);
    const CsPic p{Y, U, V, ys, uvs, w, h, rgba};
    const bool vec = ((w & 7) | (ys & 7) | (uvs & 3) | ((uintptr_t)rgba & 15) | ((uintptr_t)Y & 7) | ((uintptr_t)U & 3) | ((uintptr_t)V & 3)) == 0;
    if (vec)
        for (int u = u0; u < units; u += ustep) cs_out_unit<BIL, true>(k, p, u);
    else
        for (int u = u0; u < units; u += ustep) cs_out_unit<BIL, false>(k, p, u);
}

struct CsOutLaunch { const uint8_t *i420; uint8_t *rgba; int w, h, n; CsCoef k; };

template <bool BIL>
__global__ __launch_bounds__(256) void i420_to_rgba_cs_kernel(CsOutLaunch a) {
    const size_t ysz = (size_t)a.w * a.h, csz = (size_t)(a.w >> 1) * (a.h >> 1), fb = ysz + 2 * csz;
    const CsOut k = cs_out_coef(a.k);
    for (int f = blockIdx.y; f < a.n; f += gridDim.y) {
        const uint8_t *Y = a.i420 + (size_t)f * fb;
        i420_to_rgba_cs_picture<BIL>(k, Y, Y + ysz, Y + ysz + csz, a.w, a.w >> 1, a.w, a.h, a.rgba + (size_t)f * ysz * 4,
                                     blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
    }
}

// RGBA read-out of a batched decode call under a specification (after dec_end_kernel of frame f): what
// dec_output_rgba_kernel does, with the specification's arithmetic. The picture handed on is the cropped one, so
// BILINEAR clamps at the crop's edges and never reads a coded sample outside it. Grid (blocks, S)
struct DecCsLaunch { int S, cw, ch; const DecDesc *desc; const DecInput *in; CsCoef k; };
template <bool BIL>
__global__ __launch_bounds__(256) void dec_output_rgba_cs_kernel(DecCsLaunch a) {
    const int s = blockIdx.y;
    if (s >= a.S) return;
    const DecState *st = a.desc[s].st;
    const DecInput &I = a.in[s];
    const int ok = st->got_pic && !st->err;
    if (I.got && blockIdx.x == 0 && threadIdx.x == 0) *I.got = ok;
    if (!ok || !I.out) return;
    const int c0 = st->ps.crop[0], c1 = st->ps.crop[1], c2 = st->ps.crop[2], c3 = st->ps.crop[3];
    const int W = a.cw - 2 * (c0 + c1), H = a.ch - 2 * (c2 + c3), x0 = 2 * c0, y0 = 2 * c2;
    if (W <= 0 || H <= 0) return;
    const uint8_t *const *pic = a.desc[s].pic[st->outpar & 1];
    const int ys = a.cw, uvs = a.cw / 2;
    i420_to_rgba_cs_picture<BIL>(cs_out_coef(a.k), pic[0] + (size_t)y0 * ys + x0, pic[1] + (size_t)(y0 / 2) * uvs + x0 / 2,
                                 pic[2] + (size_t)(y0 / 2) * uvs + x0 / 2, ys, uvs, W, H, I.out, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// ---- host
// grid for n frames of w x h, color.inc's rule: every unit once when that is at most PIC_MAX_BLOCKS blocks, else a stride
// loop. Units are below 1024 * 4096 = 2^22, so the kernels' int indices hold
static dim3 cs_grid(int w, int h, int n) {
    const int ny = std::min(n, H264MI_CS_MAX_FRAMES_Y);
    const long long units = (long long)((w + 7) / 8) * (h / 2);
    const long long bx = std::max(1LL, std::min((units + 255) / 256, (long long)(PIC_MAX_BLOCKS / ny)));
    return dim3((unsigned)bx, (unsigned)ny);
}
// (each launch first drops whatever error an earlier, unrelated HIP call of the thread left behind, so that what it
// returns is its own)
int launch_rgba_to_i420_cs(uint8_t *d_out, const uint8_t *d_rgba, int w, int h, int n, const h264mi_colorspec &spec, bool alpha, hipStream_t s) {
    const CsInLaunch a{d_rgba, d_out, w, h, n, cs_coef(spec.matrix, spec.range)};
    const bool avg = spec.chroma_down == H264MI_CHROMA_DOWN_AVERAGE;
    const dim3 g = cs_grid(w, h, n);
    (void)hipGetLastError();
    if (alpha) {
        if (avg) hipLaunchKernelGGL((rgba_to_i420_cs_kernel<true, true>), g, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((rgba_to_i420_cs_kernel<false, true>), g, dim3(256), 0, s, a);
    } else {
        if (avg) hipLaunchKernelGGL((rgba_to_i420_cs_kernel<true, false>), g, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((rgba_to_i420_cs_kernel<false, false>), g, dim3(256), 0, s, a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int launch_i420_to_rgba_cs(uint8_t *d_rgba, const uint8_t *d_i420, int w, int h, int n, const h264mi_colorspec &spec, hipStream_t s) {
    const CsOutLaunch a{d_i420, d_rgba, w, h, n, cs_coef(spec.matrix, spec.range)};
    const dim3 g = cs_grid(w, h, n);
    (void)hipGetLastError();
    if (spec.chroma_up == H264MI_CHROMA_UP_BILINEAR) hipLaunchKernelGGL(i420_to_rgba_cs_kernel<true>, g, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(i420_to_rgba_cs_kernel<false>, g, dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// frame f's S entries of desc / in, as DecOutLaunch holds them; the grid is dec_output_rgba_kernel's
int launch_dec_output_rgba_cs(int S, int cw, int ch, const DecDesc *desc, const DecInput *in, const h264mi_colorspec &spec, hipStream_t s) {
    const DecCsLaunch a{S, cw, ch, desc, in, cs_coef(spec.matrix, spec.range)};
    const dim3 g(cs_grid(cw, ch, S).x, (unsigned)S);
    (void)hipGetLastError();
    if (spec.chroma_up == H264MI_CHROMA_UP_BILINEAR) hipLaunchKernelGGL(dec_output_rgba_cs_kernel<true>, g, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dec_output_rgba_cs_kernel<false>, g, dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace h264mi
