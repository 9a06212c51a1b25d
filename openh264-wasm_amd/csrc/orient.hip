// orient.hip -- rotating and mirroring tight I420 frames on the device (gfx950), as include/h264mi.h
// (h264mi_i420_orient_dev) defines it. DESIGN.md §5.9.
//   orient_rows_kernel : orientations 0, 2, 4, 5 (a destination row is a source row, maybe read backwards), no LDS
//   orient_tile_kernel : orientations 1, 3, 6, 7 (a destination row is a source column), through an LDS tile
// n frames of one geometry per launch -- the standalone call, or an encoder's source frames turned into its input
// area (h264mi_enc_encode_oriented). Every plane is turned on its own (Y sw x sh; Cb, Cr sw/2 x sh/2): samples are
// moved, never interpolated. An orientation is three bits (orient_map): whether the plane is transposed, then whether
// the destination's columns and its rows are reversed. With S the pw x ph source plane and the destination qw x qh
// (ph x pw when transposed):
//   D[y][x] = T[ry ? qh-1-y : y][rx ? qw-1-x : x],  T = S or, transposed, T[y][x] = S[x][y]
// which gives the eight rows of the header's table (ROT90 = transposed + rx, ROT270 = transposed + ry, ...).
//
// Work split. A block of four waves owns one tile of 4096 source bytes of one plane of one frame and strides over
// (frame, plane, tile); the loop count depends on the block only, so the barriers of the tile kernel are uniform.
// Both the loads and the stores of every orientation run along rows, as dwords from consecutive lanes where the
// plane allows it:
//   rows kernel: a tile is 256 samples x 16 rows. A lane loads the dwords of four rows (all four in flight), and 64
//     lanes cover 256 consecutive bytes of a row. For a reversed row (2, 4) the bytes of each dword are reversed in
//     the register (v_perm_b32 via __builtin_bswap32) and the dword goes to column pw - 4 - x: the stores of a wave
//     are again 256 consecutive bytes. For reversed rows (2, 5) the row index is mirrored.
//   tile kernel: a tile is 64 x 64 samples. 16 lanes load the 16 dwords of a source row, a wave four rows at a time,
//     into LDS. After the barrier lane (i, cd) = (t & 15, t >> 4) reads the dwords cd of source rows 4i .. 4i+3, which
//     are 4 x 4 samples, transposes them in registers with eight v_perm_b32, and holds dword i of the destination rows
//     4cd .. 4cd+3 of the transposed tile: 16 consecutive lanes store 64 consecutive bytes of a destination row. The
//     column reversal (1, 7) reverses each dword's bytes and mirrors its column, the row reversal (3, 7) mirrors the
//     row: where the tile lands and the order inside it, nothing else differs from the transpose.
//   LDS image: source row r of the tile lies in slot (r & 3) * 16 + (r >> 2), at a pitch of 18 dwords (64 slots,
//     4608 bytes a block). Derivation: ds_read_b32 serves lanes 0-31 and 32-63 as one group each, bank = dword
//     address mod 32. In a group i runs 0..15 and cd takes two consecutive values (even, odd). The read of row
//     4i + a is at dword (16 a + i) * 18 + cd, bank (18 i + cd) mod 32 (16 * 18 = 288 = 9 * 32 drops out): 18 i mod
//     32 runs through the 16 even banks once for i = 0..15, the even cd keeps them and the odd one takes the 16 odd
//     banks -- 32 lanes on 32 banks. With the rows in order at any pitch P the same read is at (4 i + a) P + cd, and
//     4 i P mod 32 has only 8 values: at least 2-way. At a pitch of 16 it is 16-way. The writes (16 lanes a row, two
//     rows r, r + 1 of one group of four in a lane group: slots 16 apart, 288 dwords, the same banks) are 2-way,
//     which costs a ds_write_b32 nothing: its four cycles are the transfer of address and data.
// Partial tiles: a tile at the right or lower edge has tw x th < 64 x 64 (256 x 16) samples; lanes beyond it load
// nothing (their LDS dwords are zero) and store nothing.
// Two paths for the same bytes, chosen per plane and frame from the plane's own pointers: a side of the move whose
// plane base and row length are multiples of 4 uses dwords; any other (a buffer at an odd address, a w % 8 != 0
// chroma) uses bytes -- a reversed row of a width that is no multiple of 4 would shift the dword boundaries, and
// takes the byte path too instead of shifting across neighbouring dwords. The tile kernel decides for its loads
// (source base, pw) and its stores (destination base, ph) separately, the rows kernel for both at once (they share
// pw). An aligned dword of a row whose length is a multiple of 4 never leaves the row, and tile origins are multiples
// of 64: no access leaves the pw x ph area of the source plane or the qw x qh area of the destination plane.
//
// A translation unit and a code object of its own, as scale.hip is: the library's other kernels stay byte for byte
// what they were. The host runtime (capi_enc.inc) reaches it through the functions picture_host.h declares.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include <string.h>
#include "../../include/h264mi.h"
#include "picture_host.h"
#include "picture_dev.h"

namespace h264mi {
#define H264MI_ORIENT_TILE 64        // tile kernel: samples each way
#define H264MI_ORIENT_PITCH 18       // dwords between two slots of the LDS image
#define H264MI_ORIENT_ROW_W 256      // rows kernel: samples across
#define H264MI_ORIENT_ROW_H 16       // rows kernel: rows

struct OrientMap { int transpose, rev_x, rev_y; };
struct OrientPlane { int pw, ph, ntx, nty; };  // source samples; tiles across / down
struct OrientLaunch {
    const uint8_t *src;
    uint8_t *dst;
    size_t fb;       // frame f: src + f * fb, dst + f * fb (turning keeps the byte count)
    size_t off[3];   // a frame's planes, the same on both sides
    int n, ntiles;   // frames; tiles per frame = luma tiles + 2 * chroma tiles
    int rev_x, rev_y;
    OrientPlane pl[2];  // luma, chroma
};

// item `it` of a launch: its frame's plane pointers, the plane's geometry and the tile's index in the plane
struct OrientItem { const uint8_t *S; uint8_t *D; OrientPlane g; int tx, ty; };
PICDEV OrientItem orient_item(const OrientLaunch &a, long long it) {
    const long long f = it / a.ntiles;
    int k = (int)(it - f * a.ntiles);
    const int lt = a.pl[0].ntx * a.pl[0].nty, ct = a.pl[1].ntx * a.pl[1].nty;
    int p = 0;
    if (k >= lt) { k -= lt; p = 1; if (k >= ct) { k -= ct; p = 2; } }
    OrientItem o;
    o.g = a.pl[p != 0];
    o.S = a.src + (size_t)f * a.fb + a.off[p];
    o.D = a.dst + (size_t)f * a.fb + a.off[p];
    o.tx = k % o.g.ntx;
    o.ty = k / o.g.ntx;
    return o;
}

__global__ __launch_bounds__(256) void orient_rows_kernel(OrientLaunch a) {
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    const long long items = (long long)a.n * a.ntiles;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const OrientItem o = orient_item(a, it);
        const int pw = o.g.pw, ph = o.g.ph;
        const int x = o.tx * H264MI_ORIENT_ROW_W + 4 * c, y0 = o.ty * H264MI_ORIENT_ROW_H + r0;
        if (x >= pw) continue;
        if (((((uintptr_t)o.S) | ((uintptr_t)o.D) | (uintptr_t)pw) & 3) == 0) {  // x + 3 < pw
            uint32_t v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int y = y0 + 4 * k;
                v[k] = y < ph ? *(const uint32_t *)(o.S + (size_t)y * pw + x) : 0u;
            }
            const int dx = a.rev_x ? pw - 4 - x : x;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int y = y0 + 4 * k;
                if (y < ph) *(uint32_t *)(o.D + (size_t)(a.rev_y ? ph - 1 - y : y) * pw + dx) = a.rev_x ? __builtin_bswap32(v[k]) : v[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int y = y0 + 4 * k;
                if (y >= ph) continue;
                const uint8_t *s = o.S + (size_t)y * pw;
                uint8_t *d = o.D + (size_t)(a.rev_y ? ph - 1 - y : y) * pw;
                for (int j = 0; j < 4 && x + j < pw; j++) d[a.rev_x ? pw - 1 - x - j : x + j] = s[x + j];
            }
        }
    }
}

// r[a] holds the samples (row a, columns 0..3) of a 4 x 4 block, column j in byte j; afterwards r[b] holds
// (column b, rows 0..3), row a in byte a. v_perm_b32: selector bytes 0..3 take the second operand's bytes, 4..7 the first's
PICDEV void transpose_4x4_bytes(uint32_t *r) {
    const uint32_t lo01 = __builtin_amdgcn_perm(r[1], r[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(r[1], r[0], 0x07030602u);
    const uint32_t lo23 = __builtin_amdgcn_perm(r[3], r[2], 0x05010400u), hi23 = __builtin_amdgcn_perm(r[3], r[2], 0x07030602u);
    r[0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
    r[1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
    r[2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
    r[3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
}

__global__ __launch_bounds__(256) void orient_tile_kernel(OrientLaunch a) {
    __shared__ uint32_t lds[H264MI_ORIENT_TILE * H264MI_ORIENT_PITCH];
    const int lo = threadIdx.x & 15, hi = threadIdx.x >> 4;  // loads: dword lo of rows hi + 16 k; stores: (i, cd)
    const long long items = (long long)a.n * a.ntiles;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {  // the same count in every thread of a block
        const OrientItem o = orient_item(a, it);
        const int pw = o.g.pw, ph = o.g.ph;  // the destination plane is ph x pw
        const int x0 = o.tx * H264MI_ORIENT_TILE, y0 = o.ty * H264MI_ORIENT_TILE;
        const int tw = min(H264MI_ORIENT_TILE, pw - x0), th = min(H264MI_ORIENT_TILE, ph - y0);
        const bool wide_src = ((((uintptr_t)o.S) | (uintptr_t)pw) & 3) == 0;  // then tw % 4 == 0
        const bool wide_dst = ((((uintptr_t)o.D) | (uintptr_t)ph) & 3) == 0;  // then th % 4 == 0
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int r = hi + 16 * k;
            v[k] = 0;
            if (r < th && 4 * lo < tw) {
                const uint8_t *s = o.S + (size_t)(y0 + r) * pw + x0 + 4 * lo;
                if (wide_src) v[k] = *(const uint32_t *)s;
                else for (int j = 0; j < 4 && 4 * lo + j < tw; j++) v[k] |= (uint32_t)s[j] << (8 * j);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int r = hi + 16 * k;
            lds[((r & 3) * 16 + (r >> 2)) * H264MI_ORIENT_PITCH + lo] = v[k];
        }
        __syncthreads();
        const int i = lo, cd = hi;  // source rows 4i .. 4i+3 (destination columns), source columns 4cd .. 4cd+3 (rows)
        uint32_t q[4];
#pragma unroll
        for (int r = 0; r < 4; r++) q[r] = lds[(r * 16 + i) * H264MI_ORIENT_PITCH + cd];
        __syncthreads();  // the image is free for the next tile
        transpose_4x4_bytes(q);
        if (4 * i < th) {
            const int col = y0 + 4 * i;  // of the transposed plane
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int j = 4 * cd + b;
                if (j >= tw) continue;
                uint8_t *d = o.D + (size_t)(a.rev_y ? pw - 1 - (x0 + j) : x0 + j) * ph;
                if (wide_dst) {
                    *(uint32_t *)(d + (a.rev_x ? ph - 4 - col : col)) = a.rev_x ? __builtin_bswap32(q[b]) : q[b];
                } else {
                    for (int r = 0; r < 4 && 4 * i + r < th; r++) d[a.rev_x ? ph - 1 - (col + r) : col + r] = (uint8_t)(q[b] >> (8 * r));
                }
            }
        }
    }
}

// ---- host
static inline bool orient_ok(int orient) { return orient >= H264MI_ORIENT_IDENTITY && orient <= H264MI_ORIENT_TRANSVERSE; }
static OrientMap orient_map(int orient) {
    static const OrientMap m[8] = {{0, 0, 0}, {1, 1, 0}, {0, 1, 1}, {1, 0, 1}, {0, 1, 0}, {0, 0, 1}, {1, 0, 0}, {1, 1, 1}};
    return m[orient];
}
// arguments of an orient call: a known orientation, even sides from 2 within PIC_MAX_SIDE, n >= 1
bool orient_args_ok(int orient, int sw, int sh, int n) { return n > 0 && orient_ok(orient) && canvas_ok(sw, sh); }
int orient_size(int orient, int sw, int sh, int *dw, int *dh) {
    if (!dw || !dh || !orient_ok(orient) || !canvas_ok(sw, sh)) return -1;
    const bool t = orient_map(orient).transpose != 0;
    *dw = t ? sh : sw;
    *dh = t ? sw : sh;
    return 0;
}
// the definition on the host, one plane: the pw x ph samples at S turned into D; what compose and inverse are read from
void orient_plane_host(int orient, const uint8_t *S, int pw, int ph, uint8_t *D) {
    const OrientMap m = orient_map(orient);
    const int qw = m.transpose ? ph : pw, qh = m.transpose ? pw : ph;
    for (int y = 0; y < qh; y++)
        for (int x = 0; x < qw; x++) {
            const int u = m.rev_x ? qw - 1 - x : x, v = m.rev_y ? qh - 1 - y : y;
            D[y * qw + x] = m.transpose ? S[u * pw + v] : S[v * pw + u];
        }
}
// the orientation that equals `first`, then `then`: both applied to a 3 x 2 plane of six different samples, which tells
// all eight apart, and the result looked up among the eight
int orient_compose(int first, int then) {
    if (!orient_ok(first) || !orient_ok(then)) return -1;
    const uint8_t P[6] = {0, 1, 2, 3, 4, 5};
    uint8_t A[6], B[6], C[6];
    const bool t1 = orient_map(first).transpose != 0, t2 = orient_map(then).transpose != 0;
    orient_plane_host(first, P, 3, 2, A);
    orient_plane_host(then, A, t1 ? 2 : 3, t1 ? 3 : 2, B);
    for (int k = 0; k < 8; k++) {
        if ((orient_map(k).transpose != 0) != (t1 != t2)) continue;
        orient_plane_host(k, P, 3, 2, C);
        if (memcmp(B, C, 6) == 0) return k;
    }
    return -1;  // not reached: the eight are closed under composition
}
int orient_inverse(int orient) {
    for (int k = 0; k < 8; k++)
        if (orient_compose(orient, k) == H264MI_ORIENT_IDENTITY) return k;
    return -1;  // a bad orientation
}
static OrientPlane orient_plane(int pw, int ph, int tile_w, int tile_h) {
    return OrientPlane{pw, ph, (pw + tile_w - 1) / tile_w, (ph + tile_h - 1) / tile_h};
}
// n tight sw x sh I420 frames at src turned into n tight frames at dst; arguments as orient_args_ok accepts them
int launch_orient_i420(uint8_t *dst, const uint8_t *src, int sw, int sh, int n, int orient, hipStream_t s) {
    const OrientMap m = orient_map(orient);
    const int tile_w = m.transpose ? H264MI_ORIENT_TILE : H264MI_ORIENT_ROW_W, tile_h = m.transpose ? H264MI_ORIENT_TILE : H264MI_ORIENT_ROW_H;
    const size_t ly = (size_t)sw * sh, lc = (size_t)(sw / 2) * (sh / 2);
    OrientLaunch a{};
    a.src = src; a.dst = dst; a.fb = ly + 2 * lc;
    a.off[0] = 0; a.off[1] = ly; a.off[2] = ly + lc;
    a.n = n;
    a.rev_x = m.rev_x; a.rev_y = m.rev_y;
    a.pl[0] = orient_plane(sw, sh, tile_w, tile_h);
    a.pl[1] = orient_plane(sw / 2, sh / 2, tile_w, tile_h);
    a.ntiles = a.pl[0].ntx * a.pl[0].nty + 2 * a.pl[1].ntx * a.pl[1].nty;  // at most 24576 (8192 x 8192)
    const unsigned blocks = (unsigned)std::min((long long)n * a.ntiles, (long long)PIC_MAX_BLOCKS);
    (void)hipGetLastError();
    if (m.transpose) hipLaunchKernelGGL(orient_tile_kernel, dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(orient_rows_kernel, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace h264mi
