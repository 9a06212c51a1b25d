// enc_planes.inc -- the encoder's motion-search reference planes (gfx950).
//
// After a frame is deblocked (the next frame's reference, 8.4.2.2), one fully parallel pass builds
// the four luma sample planes the motion search reads -- G (integer), b (horizontal half sample),
// h (vertical half), j (centre half) -- and the two chroma planes, all edge-padded:
//   G(x, y) = ref(clip(x), clip(y))                              (8-228 / 8-229 reference padding)
//   b(x, y) = Clip1((tap6 of G(x-2..x+3, y)) + 16) >> 5          (8-241, 8-243)
//   h(x, y) = Clip1((tap6 of G(x, y-2..y+3)) + 16) >> 5          (8-242, 8-244)
//   j(x, y) = Clip1((tap6 of b1(x, y-2..y+3)) + 512) >> 10,  b1 = unrounded horizontal tap (8-245/8-247)
// so quarter samples are a rounded average of two plane samples (8-250..8-261, qsel() in
// enc_mb.inc) and the MB wavefront never interpolates on its critical path. HBM-bound: reads the
// picture once, writes 4 padded luma + 2 padded chroma planes (~10 MB per 1080p stream). These blocks
// run inside enc_post_kernel (below).
// The decoder does not use b, h, j: dec_planes_kernel (below) pads G and chroma only, in the same
// geometry, and dec_recon.inc filters at the point of use.
namespace h264mi {

// ystrips: luma row strips (blockIdx.y below it); the blocks above it copy the padded chroma planes
struct PlanesLaunch { int S, cw, ch; const PlanesDesc *pd; int ystrips; };

// Luma: a thread owns one 4-sample column quad of the padded plane over PT_H rows. Picture loads
// (three aligned dwords per row, x-4..x+7, edge-clamped per quad) run one row
// ahead of the output row; the thread slides a six-row window down the quad in registers: the unrounded horizontal taps b1 of each row, G/b/h/j of the output row ->
// four coalesced dword stores per row. Reads the picture ~1.3 times, writes each plane once
// (HBM-bound). The padded height ch + 2 * LPADY is a multiple of PT_H (ch is the coded height).
// blockIdx.y = row strip, blockIdx.z = stream.
constexpr int PT_H = 16, PT_Q = 256;  // rows per thread, column quads per workgroup
static_assert((2 * H264MI_LPADY) % PT_H == 0, "planes strips tile the padded height");
// bytes x..x+3 of an edge-clamped picture row, x a multiple of 4: the picture width is a multiple of
// 16, so a quad lies wholly inside the row or wholly beyond one end (then it repeats the end sample)
DEV uint32_t planes_row_bytes(const uint8_t *row, int x, int cw) {
    const uint32_t v = *(const uint32_t *)(row + clip3(0, cw - 4, x));
    return x < 0 ? (v & 255u) * 0x01010101u : (x >= cw ? (v >> 24) * 0x01010101u : v);
}
DEV void ref_planes_chroma(const PlanesLaunch &a, const PlanesDesc &D, int i);
// block (bx, by, bz) of a gx-wide grid: by < ystrips luma strips, above them the chroma copies; bz = stream
DEV void ref_planes_block(const PlanesLaunch &a, int bx, int by, int bz, int gx) {
    const PlanesDesc &D = a.pd[bz];
    if (D.active && *D.active == 0) return;
    if (by >= a.ystrips) {  // chroma blocks of the same launch (one dispatch per picture)
        ref_planes_chroma(a, D, ((by - a.ystrips) * gx + bx) * PT_Q + (int)threadIdx.x);
        return;
    }
    const int cw = a.cw, ch = a.ch;
    const int pw = cw + 2 * H264MI_LPADX;
    const int q = bx * PT_Q + (int)threadIdx.x;
    if (q * 4 >= pw) return;
    const int x0 = q * 4 - H264MI_LPADX;                  // first sample of the quad (plane coordinates)
    const int ya = by * PT_H - H264MI_LPADY;               // first output row
    const uint8_t *ref = D.src[D.parity ? (*D.parity & 1) : 0][0];
    // six-row window (G quads and unrounded horizontal taps b1 (8-241) of samples x0..x0+3 as int16
    // pairs) plus one row of loads in flight; the loop is not unrolled so the window stays in ~30
    // registers and the kernel co-resides with the wavefront kernels (<= 64 VGPRs)
    uint32_t Mw[6], Bw[6][2], qL, qM, qR;
    auto issue = [&](int i) {  // picture row ya - 2 + i
        const uint8_t *row = ref + (size_t)clip3(0, ch - 1, ya - 2 + i) * cw;
        qL = planes_row_bytes(row, x0 - 4, cw);
        qM = planes_row_bytes(row, x0, cw);
        qR = planes_row_bytes(row, x0 + 4, cw);
    };
    auto absorb = [&](int slot) {  // samples x0-2 .. x0+6 of the loaded row -> window slot
        const uint32_t lo = __builtin_amdgcn_alignbyte(qM, qL, 2), hi = __builtin_amdgcn_alignbyte(qR, qM, 2);
        int sm[9];
        sm[0] = lo & 255; sm[1] = (lo >> 8) & 255; sm[2] = (lo >> 16) & 255; sm[3] = lo >> 24;
        sm[4] = hi & 255; sm[5] = (hi >> 8) & 255; sm[6] = (hi >> 16) & 255; sm[7] = hi >> 24; sm[8] = (qR >> 16) & 255;
        int t[4];  // |t| < 2^14
#pragma unroll
        for (int k = 0; k < 4; k++) t[k] = tap6(sm[k], sm[k + 1], sm[k + 2], sm[k + 3], sm[k + 4], sm[k + 5]);
        Mw[slot] = qM;
        Bw[slot][0] = (uint32_t)(t[0] & 0xffff) | ((uint32_t)t[1] << 16);
        Bw[slot][1] = (uint32_t)(t[2] & 0xffff) | ((uint32_t)t[3] << 16);
    };
    auto b1 = [&](int i, int k) -> int { return __builtin_amdgcn_sbfe((int)Bw[i][k >> 1], 16 * (k & 1), 16); };
#pragma unroll
    for (int i = 0; i < 5; i++) { issue(i); absorb(i); }
    issue(5);
    uint8_t *pG = D.pl[0], *pB = D.pl[1], *pH = D.pl[2], *pJ = D.pl[3];
#pragma unroll 1
    for (int r = 0; r < PT_H; r++) {  // output row ya + r = window slot 2
        absorb(5);
        if (r + 1 < PT_H) issue(r + 6);
        uint32_t vb = 0, vh = 0, vj = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int sh = 8 * k;
            const int Hv = tap6((Mw[0] >> sh) & 255, (Mw[1] >> sh) & 255, (Mw[2] >> sh) & 255, (Mw[3] >> sh) & 255,
                                (Mw[4] >> sh) & 255, (Mw[5] >> sh) & 255);
            const int J = tap6(b1(0, k), b1(1, k), b1(2, k), b1(3, k), b1(4, k), b1(5, k));
            vb |= (uint32_t)clip1_shr(b1(2, k) + 16, 5) << sh;
            vh |= (uint32_t)clip1_shr(Hv + 16, 5) << sh;
            vj |= (uint32_t)clip1_shr(J + 512, 10) << sh;
        }
        const ptrdiff_t o = (ptrdiff_t)(ya + r) * D.ps + x0;
        *(uint32_t *)(pG + o) = Mw[2];
        *(uint32_t *)(pB + o) = vb;
        *(uint32_t *)(pH + o) = vh;
        *(uint32_t *)(pJ + o) = vj;
#pragma unroll
        for (int i = 0; i < 5; i++) { Mw[i] = Mw[i + 1]; Bw[i][0] = Bw[i + 1][0]; Bw[i][1] = Bw[i + 1][1]; }
    }
}

// Chroma: edge-replicated copies, four samples per thread and dword, PT_H rows per thread: thread i of the
// chroma blocks -> plane, row strip, column quad (consecutive threads: consecutive quads of a row); CPADX
// and the chroma width are multiples of 4, so a quad lies wholly inside the row or wholly beyond one end
// (planes_row_bytes).
DEV void ref_planes_chroma(const PlanesLaunch &a, const PlanesDesc &D, int i) {
    const int cwc = a.cw / 2, chc = a.ch / 2;
    const int pw = cwc + 2 * H264MI_CPADX, ph = chc + 2 * H264MI_CPADY, q = pw / 4, strips = (ph + PT_H - 1) / PT_H;
    const int pl = i / (q * strips);
    if (pl >= 2) return;
    i -= pl * q * strips;
    const int st = i / q, xx = (i - st * q) * 4, x = xx - H264MI_CPADX;
    static_assert(H264MI_CPADX % 4 == 0, "chroma quads are dword-aligned");
    const uint8_t *base = D.src[D.parity ? (*D.parity & 1) : 0][1 + pl];
#pragma unroll 1
    for (int r = 0; r < PT_H; r++) {
        const int yy = st * PT_H + r;
        if (yy >= ph) break;
        const int y = yy - H264MI_CPADY;
        *(uint32_t *)(D.plc[pl] + (ptrdiff_t)y * D.psc + x) = planes_row_bytes(base + (size_t)clip3(0, chc - 1, y) * cwc, x, cwc);
    }
}

static void ref_planes_grid(int cw, int ch, int &gx, int &gy, int &ystrips) {
    const int quads = (cw + 2 * H264MI_LPADX) / 4;
    gx = (quads + PT_Q - 1) / PT_Q;
    ystrips = (ch + 2 * H264MI_LPADY + PT_H - 1) / PT_H;
    const int cq = 2 * ((cw / 2 + 2 * H264MI_CPADX) / 4) * ((ch / 2 + 2 * H264MI_CPADY + PT_H - 1) / PT_H);  // chroma threads
    gy = ystrips + (cq + gx * PT_Q - 1) / (gx * PT_Q);
}
// The decoder's reference planes: the edge-padded integer plane G (D.pl[0]; pl[1..3] are not touched and may
// be null) and the two padded chroma planes, in the geometry above and on the same grid -- a padding copy, no
// taps. The decoder's reconstruction samples every block once at a known vector and runs the six-tap filters
// where a vector is fractional (dec_recon.inc), so the b / h / j planes would be written (6.9 MB per 1080p
// stream and frame) for nothing. A thread copies its column quad over the strip's PT_H rows, all loads first.
__global__ __launch_bounds__(PT_Q) void dec_planes_kernel(PlanesLaunch a) {
    const PlanesDesc &D = a.pd[blockIdx.z];
    if (D.active && *D.active == 0) return;
    if ((int)blockIdx.y >= a.ystrips) {
        ref_planes_chroma(a, D, (((int)blockIdx.y - a.ystrips) * (int)gridDim.x + (int)blockIdx.x) * PT_Q + (int)threadIdx.x);
        return;
    }
    const int cw = a.cw, ch = a.ch;
    const int q = (int)blockIdx.x * PT_Q + (int)threadIdx.x;
    if (q * 4 >= cw + 2 * H264MI_LPADX) return;
    const int x0 = q * 4 - H264MI_LPADX, ya = (int)blockIdx.y * PT_H - H264MI_LPADY;  // the quad's first sample, the first row
    const uint8_t *ref = D.src[D.parity ? (*D.parity & 1) : 0][0];
    uint32_t v[PT_H];
#pragma unroll
    for (int r = 0; r < PT_H; r++) v[r] = planes_row_bytes(ref + (size_t)clip3(0, ch - 1, ya + r) * cw, x0, cw);
#pragma unroll
    for (int r = 0; r < PT_H; r++) *(uint32_t *)(D.pl[0] + (ptrdiff_t)(ya + r) * D.ps + x0) = v[r];
}
static int launch_dec_planes(int S, int cw, int ch, const PlanesDesc *pd, hipStream_t st) {
    int gx, gy, ystrips;
    ref_planes_grid(cw, ch, gx, gy, ystrips);
    const PlanesLaunch pla{S, cw, ch, pd, ystrips};
    hipLaunchKernelGGL(dec_planes_kernel, dim3(gx, gy, S), dim3(PT_Q), 0, st, pla);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The encoder's step after enc_mb_kernel, one launch: blocks [0, S) pack the streams' slices (and update
// the rate control), the rest build the next frame's reference planes -- the two depend only on
// enc_mb_kernel, and each launch behind the wavefront grids waits for CU slots, so one dispatch instead
// of two (the packing no longer delays the planes either).
static_assert(PACK_THREADS == PT_Q, "enc_post_kernel: one block size");
struct PostLaunch { PackLaunch pk; PlanesLaunch pl; int gx, gy; };
__global__ __launch_bounds__(PT_Q) void enc_post_kernel(PostLaunch a) {
    const int b = (int)blockIdx.x;
    if (b < a.pk.S) { enc_pack_block(a.pk, b); return; }
    const int r = b - a.pk.S, per = a.gx * a.gy, z = r / per, yx = r - z * per, y = yx / a.gx;
    ref_planes_block(a.pl, yx - y * a.gx, y, z, a.gx);
}
// the same with the multi-slice pack (enc_pack_block_slices): a kernel of its own, so that its registers do not
// count against the default single-slice step
__global__ __launch_bounds__(PT_Q) void enc_post_slices_kernel(PostLaunch a) {
    const int b = (int)blockIdx.x;
    if (b < a.pk.S) { enc_pack_block_slices(a.pk, b); return; }
    const int r = b - a.pk.S, per = a.gx * a.gy, z = r / per, yx = r - z * per, y = yx / a.gx;
    ref_planes_block(a.pl, yx - y * a.gx, y, z, a.gx);
}
static int launch_enc_post(const PackLaunch &pk, int cw, int ch, const PlanesDesc *pd, hipStream_t st, bool slices) {
    int gx, gy, ystrips;
    ref_planes_grid(cw, ch, gx, gy, ystrips);
    const PostLaunch pl{pk, PlanesLaunch{pk.S, cw, ch, pd, ystrips}, gx, gy};
    if (slices) hipLaunchKernelGGL(enc_post_slices_kernel, dim3(pk.S + gx * gy * pk.S), dim3(PT_Q), 0, st, pl);
    else hipLaunchKernelGGL(enc_post_kernel, dim3(pk.S + gx * gy * pk.S), dim3(PT_Q), 0, st, pl);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace h264mi
