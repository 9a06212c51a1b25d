// enc_mb_kernel.inc -- residual coding, intra/inter decisions and the MB-row wavefront kernel.
// Continues enc_mb.inc (same namespace, same LDS image).
namespace h264mi {

// ---------------------------------------------------------------- residual coding of a whole MB
// Lane per coefficient: luma block b = tid >> 4 on all 256 threads (unless do_luma == 0: I4 MBs code
// luma block by block in the search chain), chroma block (plane, b) on threads 0..127; lane & 15 is
// the raster position inside the 4x4 block (h264mi_dev.h: xf_*). Computes levels (scan order) into
// S.lvl / S.ldc / S.cdc, TotalCoeff into S.nnz and, if recon, the reconstruction into S.rec / S.recc.
// Returns cbp (luma | chroma << 4), uniform. DESIGN.md §3.4.
// Inter / I4-chroma variant (no luma DC transform): every value a lane needs is produced on its own
// wave -- luma block row w and chroma plane w (w < 2) live on wave w, as do the prediction samples
// fill_pred_mv / chroma_mc wrote for them -- so the chroma DC transforms run on uniform registers
// (readlane of the four DC lanes), the reconstruction follows the levels directly, and one barrier
// at the end publishes levels, TotalCoeff and reconstruction. Same results as code_residual.
DEV int code_residual_nodc(EncLds &S, const Xf &X, int qp, int intra, int do_luma, bool recon) {
    const int tid = e_tid(), pos = tid & 15, lane = tid & 63;
    const QuantQP q = make_qqp(qp), qc = make_qqp(c_CHROMA_QP[qp]);
    const int fl = qff(q, X.cls, intra), fc = qff(qc, X.cls, intra), fc0 = intra ? qc.fi0 : qc.fp0;
    const int lb = tid >> 4, lx = (lb & 3) * 4 + (pos & 3), ly = (lb >> 2) * 4 + (pos >> 2);
    if (do_luma) {
        const int pv = S.pred[ly * 16 + lx];
        const int t = xf_fwd(S.src[ly * 16 + lx] - pv, X);
        const int mf = X.cls == 0 ? q.mf0 : (X.cls == 1 ? q.mf1 : q.mf2);
        const int lv = quant1(t, mf, fl);
        S.lvl[lb][X.zz] = (int16_t)lv;
        const uint64_t m = __ballot(lv != 0);
        if (pos == 0) S.nnz[lb] = (int)popc((m >> (16 * (lb & 3))) & 0xffffu);
        if (recon) {
            const int v = X.cls == 0 ? q.v0 : (X.cls == 1 ? q.v1 : q.v2);
            const int r = (xf_inv((lv * v) << q.q6, X) + 32) >> 6;
            S.rec[ly * 16 + lx] = (uint8_t)clip1(pv + r);
        }
    }
    if (tid < 128) {  // wave 0: Cb, wave 1: Cr; block cb on lanes 16 cb .. 16 cb + 15
        const int cp = tid >> 6, cb = (tid >> 4) & 3, cx = (cb & 1) * 4 + (pos & 3), cy = (cb >> 1) * 4 + (pos >> 2);
        const int pv = S.predc[cp][cy * 8 + cx];
        const int t = xf_fwd(S.srcc[cp][cy * 8 + cx] - pv, X);
        const int mf = X.cls == 0 ? qc.mf0 : (X.cls == 1 ? qc.mf1 : qc.mf2);
        const int lvc = pos == 0 ? 0 : quant1(t, mf, fc);
        S.lvl[16 + 4 * cp + cb][X.zz] = (int16_t)lvc;
        const uint64_t mc = __ballot(lvc != 0);
        if (pos == 0) S.nnz[16 + 4 * cp + cb] = (int)popc((mc >> (16 * cb)) & 0xffffu);
        // 2x2 DC Hadamard + quantisation, uniform (8.5.11 inverse below)
        const int a = lane_read(t, 0), b = lane_read(t, 16), e = lane_read(t, 32), g = lane_read(t, 48);
        const int c0 = quant_dc(a + b + e + g, qc.mf0, fc0), c1 = quant_dc(a - b + e - g, qc.mf0, fc0);
        const int c2 = quant_dc(a + b - e - g, qc.mf0, fc0), c3 = quant_dc(a - b - e + g, qc.mf0, fc0);
        if (lane == 0) {
            S.cdc[cp][0] = (int16_t)c0; S.cdc[cp][1] = (int16_t)c1; S.cdc[cp][2] = (int16_t)c2; S.cdc[cp][3] = (int16_t)c3;
        }
        if (recon) {
            const int f = cb == 0 ? c0 + c1 + c2 + c3 : cb == 1 ? c0 - c1 + c2 - c3 : cb == 2 ? c0 + c1 - c2 - c3 : c0 - c1 - c2 + c3;
            const int v = X.cls == 0 ? qc.v0 : (X.cls == 1 ? qc.v1 : qc.v2);
            const int w = pos == 0 ? ((f * qc.v0) << qc.q6) >> 1 : (lvc * v) << qc.q6;
            const int r = (xf_inv(w, X) + 32) >> 6;
            S.recc[cp][cy * 8 + cx] = (uint8_t)clip1(pv + r);
        }
    }
    lds_barrier();
    // coded_block_pattern from one ballot: lanes 0..15 luma TotalCoeff, 16..23 chroma AC, 24..31 chroma DC
    const int probe = lane < 24 ? S.nnz[lane] : (lane < 32 ? S.cdc[(lane - 24) >> 2][(lane - 24) & 3] : 0);
    const uint32_t nzb = (uint32_t)__ballot(probe != 0);
    const int lum = ((nzb & 0x0033u) ? 1 : 0) | ((nzb & 0x00ccu) ? 2 : 0) | ((nzb & 0x3300u) ? 4 : 0) | ((nzb & 0xcc00u) ? 8 : 0);
    const int cbpc = (nzb & 0x00ff0000u) ? 2 : ((nzb & 0xff000000u) ? 1 : 0);
    return uni(lum | (cbpc << 4));
}
DEV int code_residual(EncLds &S, const Xf &X, int qp, int i16, int intra, int do_luma, bool recon = true) {
    const int tid = e_tid(), pos = tid & 15, lane = tid & 63;
    const QuantQP q = make_qqp(qp), qc = make_qqp(c_CHROMA_QP[qp]);
    const int fl = qff(q, X.cls, intra), fc = qff(qc, X.cls, intra), fc0 = intra ? qc.fi0 : qc.fp0;
    // luma coefficient of this lane
    const int lb = tid >> 4, lx = (lb & 3) * 4 + (pos & 3), ly = (lb >> 2) * 4 + (pos >> 2);
    int lv = 0;
    if (do_luma) {
        const int d = S.src[ly * 16 + lx] - S.pred[ly * 16 + lx];
        const int t = xf_fwd(d, X);
        if (i16 && pos == 0) S.dcraw[lb] = t;
        const int mf = X.cls == 0 ? q.mf0 : (X.cls == 1 ? q.mf1 : q.mf2);
        lv = (i16 && pos == 0) ? 0 : quant1(t, mf, fl);
        S.lvl[lb][X.zz] = (int16_t)lv;
        const uint64_t m = __ballot(lv != 0);
        if (pos == 0) S.nnz[lb] = (int)popc((m >> (16 * (lb & 3))) & 0xffffu);
    }
    // chroma coefficient (threads 0..127): plane cp, block cb
    const bool isc = tid < 128;
    const int cp = (tid >> 6) & 1, cb = (tid >> 4) & 3, cx = (cb & 1) * 4 + (pos & 3), cy = (cb >> 1) * 4 + (pos >> 2);
    int lvc = 0;
    if (isc) {
        const int d = S.srcc[cp][cy * 8 + cx] - S.predc[cp][cy * 8 + cx];
        const int t = xf_fwd(d, X);
        if (pos == 0) S.dcraw[16 + 4 * cp + cb] = t;
        const int mf = X.cls == 0 ? qc.mf0 : (X.cls == 1 ? qc.mf1 : qc.mf2);
        lvc = pos == 0 ? 0 : quant1(t, mf, fc);
        S.lvl[16 + 4 * cp + cb][X.zz] = (int16_t)lvc;
    }
    const uint64_t mc = __ballot(lvc != 0);
    if (isc && pos == 0) S.nnz[16 + 4 * cp + cb] = (int)popc((mc >> (16 * cb)) & 0xffffu);
    lds_barrier();
    if (tid < 16 && i16) {  // forward 4x4 Hadamard of the luma DC matrix (lane = 4 * block row + block column),
        // (x + 1) >> 1 as OpenH264's WelsHadamardT4Dc (h264.wasm func 1029), quantise (intra rounding)
        const int F = (xf_had(S.dcraw[tid], X) + 1) >> 1;
        S.ldc[X.zz] = (int16_t)quant_dc(F, q.mf0, q.fi0);
    }
    if (tid >= 16 && tid < 24) {  // 2x2 chroma DC Hadamard + quantise
        const int pl = (tid - 16) >> 2, k = (tid - 16) & 3;
        const int a = S.dcraw[16 + 4 * pl], b = S.dcraw[17 + 4 * pl], e = S.dcraw[18 + 4 * pl], g = S.dcraw[19 + 4 * pl];
        const int f = k == 0 ? a + b + e + g : k == 1 ? a - b + e - g : k == 2 ? a + b - e - g : a - b - e + g;
        S.cdc[pl][k] = (int16_t)quant_dc(f, qc.mf0, fc0);
    }
    lds_barrier();
    // coded_block_pattern from one ballot: lanes 0..15 luma TotalCoeff, 16..23 chroma AC, 24..31 chroma DC
    const int probe = lane < 24 ? S.nnz[lane] : (lane < 32 ? S.cdc[(lane - 24) >> 2][(lane - 24) & 3] : 0);
    const uint64_t nzm = __ballot(probe != 0);
    const uint32_t nzb = (uint32_t)nzm;
    int lum = ((nzb & 0x0033u) ? 1 : 0) | ((nzb & 0x00ccu) ? 2 : 0) | ((nzb & 0x3300u) ? 4 : 0) | ((nzb & 0xcc00u) ? 8 : 0);
    if (i16) lum = lum ? 15 : 0;
    const int cbpc = (nzb & 0x00ff0000u) ? 2 : ((nzb & 0xff000000u) ? 1 : 0);
    const int cbp = uni(lum | (cbpc << 4));
    if (!recon) return cbp;  // decision only (P_Skip test): levels, nnz and cbp
    // DC inverse transforms (8.5.10, 8.5.11)
    if (tid < 16 && i16) S.dcval[tid] = luma_dc_scale(xf_had(S.ldc[X.zz], X), q);
    if (tid >= 16 && tid < 24) {
        const int pl = (tid - 16) >> 2, k = (tid - 16) & 3;
        const int a = S.cdc[pl][0], b = S.cdc[pl][1], e = S.cdc[pl][2], g = S.cdc[pl][3];
        const int f = k == 0 ? a + b + e + g : k == 1 ? a - b + e - g : k == 2 ? a + b - e - g : a - b - e + g;
        S.dcval[16 + 4 * pl + k] = ((f * qc.v0) << qc.q6) >> 1;
    }
    lds_barrier();
    if (do_luma) {  // dequantise (8.5.12.1), inverse transform, add the prediction
        const int v = X.cls == 0 ? q.v0 : (X.cls == 1 ? q.v1 : q.v2);
        int w = (lv * v) << q.q6;
        if (i16 && pos == 0) w = S.dcval[lb];
        const int r = (xf_inv(w, X) + 32) >> 6;
        S.rec[ly * 16 + lx] = (uint8_t)clip1(S.pred[ly * 16 + lx] + r);
    }
    if (isc) {
        const int v = X.cls == 0 ? qc.v0 : (X.cls == 1 ? qc.v1 : qc.v2);
        int w = (lvc * v) << qc.q6;
        if (pos == 0) w = S.dcval[16 + 4 * cp + cb];
        const int r = (xf_inv(w, X) + 32) >> 6;
        S.recc[cp][cy * 8 + cx] = (uint8_t)clip1(S.predc[cp][cy * 8 + cx] + r);
    }
    lds_barrier();
    return cbp;
}

// ---------------------------------------------------------------- intra 16x16 prediction (8.3.3)
struct I16Ctx { int dc, a, b, c, has_top, has_left; };
// 8.3.3 context (DC value, plane parameters) from S.top / S.left: the sums on lanes 0..15 of every
// wave (DPP reductions), results uniform
template <class LDS> DEV I16Ctx i16_ctx(const LDS &S, int has_top, int has_left) {
    const int l = e_tid() & 15;
    const int st = S.top[1 + l], sl = S.left[l];
    const int hh = l < 8 ? (l + 1) * (S.top[9 + l] - S.top[7 - l]) : 0;
    const int vv = l < 8 ? (l + 1) * (S.left[8 + l] - (l < 7 ? S.left[6 - l] : S.top[0])) : 0;
    const int sumt = lane_read(group16_sum(st), 0), suml = lane_read(group16_sum(sl), 0);
    const int H = lane_read(group16_sum(hh), 0), V = lane_read(group16_sum(vv), 0);
    I16Ctx r;
    if (has_top && has_left) r.dc = (sumt + suml + 16) >> 5;
    else if (has_left) r.dc = (suml + 8) >> 4;
    else if (has_top) r.dc = (sumt + 8) >> 4;
    else r.dc = 128;
    r.a = uni(16 * (S.left[15] + S.top[16])); r.b = (5 * H + 32) >> 6; r.c = (5 * V + 32) >> 6;
    r.has_top = has_top; r.has_left = has_left;
    return r;
}
template <class LDS> DEV int i16_pred(const LDS &S, const I16Ctx &k, int mode, int x, int y) {
    int vh = mode == 0 ? S.top[1 + x] : S.left[y];
    int pln = clip1((k.a + k.b * (x - 7) + k.c * (y - 7) + 16) >> 5);
    return mode <= 1 ? vh : (mode == 2 ? k.dc : pln);
}
DEV bool i16_avail(const I16Ctx &k, int m) {
    return m == 2 || (m == 0 && k.has_top) || (m == 1 && k.has_left) || (m == 3 && k.has_top && k.has_left);
}
DEV void i16_fill_pred(EncLds &S, const I16Ctx &k, int mode) {
    for (int i = e_tid(); i < 256; i += ENC_THREADS) S.pred[i] = (uint8_t)i16_pred(S, k, mode, i & 15, i >> 4);
    lds_barrier();
}

// ---------------------------------------------------------------- OpenH264's intra mode decision (DESIGN.md §3.3)
// At the wrapper's settings (camera usage, complexity LOW) OpenH264 costs modes by SAD (pfMdCost = pfSampleSad,
// h264.wasm func 1017 675945-675956) plus lambda x the mode's bits, tries them in its tables' order and keeps the
// first minimum. Tables as the oracle's (oracle/h264o_tables.h, pinned to the binary by tests/test_oracle_golden.py).
// I16x16 / chroma: the internal modes of [neighbour flags & 7] (flags: 1 left, 2 top, 4 top-left, 8 top-right)
// already mapped to syntax modes (the internal DC_L / DC_T / DC_128 are the standard's DC for those neighbours),
// count in column 4.
// The I16x16 / chroma orders as packed immediates (mode k in bits 4k..4k+3, the count in bits 16..19), chosen by a
// switch: no memory access -- a constant-table load inside the MB loop costs a vmcnt wait on the previous MB's output
// stores. I16x16 (g_kiIntra16AvaliMode mapped to syntax modes): {DC}, {DC, H}, {DC, V}, {V, H, DC}, {V, H, DC, P} for
// flags & 7 = 0 / 4, 1 / 5, 2 / 6, 3, 7; chroma (g_kiIntraChromaAvailMode): {DC}, {DC, H}, {DC, V}, {V, H, DC},
// {V, H, DC, P} -- syntax modes DC 0, H 1, V 2, P 3
DEV uint32_t md_i16_order(int flags) {
    switch (flags & 7) {
    case 1: case 5: return 0x20012u;
    case 2: case 6: return 0x20002u;
    case 3: return 0x30210u;
    case 7: return 0x43210u;
    default: return 0x10002u;
    }
}
DEV uint32_t md_chroma_order(int flags) {
    switch (flags & 7) {
    case 1: case 5: return 0x20010u;
    case 2: case 6: return 0x20020u;
    case 3: return 0x30012u;
    case 7: return 0x43012u;
    default: return 0x10000u;
    }
}
// Intra4x4: the availability index of block b (decoding order) of an MB with neighbour flags f, the number of modes
// it tries, and (fewer than 7) the syntax modes in order; 7 or 9 take WelsMdI4x4Fast's fast search (i4_choose)
// Nibble-packed (entry k at bits 4k) so that every lookup is a scalar load or an immediate: the byte tables they
// replace were read with vector loads (no scalar byte loads), each waited for with vmcnt(0) -- behind the MB's
// prefetch and the previous MB's output stores -- three times per 4x4 block of the Intra4x4 search.
// c_MD_I4_IDX4[f]: block b's availability index; MD_I4_CNT4: modes tried per index; c_MD_I4_LIST4[i]: the modes in order
__constant__ uint64_t c_MD_I4_IDX4[16] = {
    0x7f7f7afa7f117a10ull, 0x7f7f7fff7f117f11ull, 0x7f7f7afa7f7f7afaull, 0x7f7f7fff7f7f7ffbull, 0x7f7f7afa7f117a14ull,
    0x7f7f7fff7f117f15ull, 0x7f7f7afa7f7f7afeull, 0x7f7f7fff7f7f7fffull, 0x7f7f7afa7f917a10ull, 0x7f7f7fff7f917f11ull,
    0x7f7f7afa7fff7afaull, 0x7f7f7fff7fff7ffbull, 0x7f7f7afa7f917a14ull, 0x7f7f7fff7f917f15ull, 0x7f7f7afa7fff7afeull,
    0x7f7f7fff7fff7fffull};
constexpr uint64_t MD_I4_CNT4 = 0x9431643172314231ull;  // {1, 3, 2, 4, 1, 3, 2, 7, 1, 3, 4, 6, 1, 3, 4, 9}
__constant__ uint32_t c_MD_I4_LIST4[16] = {0x2u, 0x812u, 0x2u, 0x8012u, 0x2u, 0x812u, 0x2u, 0x0u,
                                           0x2u, 0x812u, 0x7302u, 0x738012u, 0x2u, 0x812u, 0x7302u, 0x0u};
DEV int ue_bits(int v) { return 2 * (31 - __clz(v + 1)) + 1; }
// the first minimum of cost[m] + lam * ue_bits(m) over the syntax modes of the packed order ord (uniform)
DEV int md_first_min(uint32_t ord, const int *cost, int lam, int *best) {
    const int n = (int)(ord >> 16);
    int b = 0x7fffffff, bm = (int)(ord & 15u);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int m = (int)((ord >> (4 * i)) & 15u);
        const int cm = m == 0 ? cost[0] : (m == 1 ? cost[1] : (m == 2 ? cost[2] : cost[3]));  // selects, no scratch
        const int c = cm + lam * ue_bits(m);
        if (i < n && c < b) { b = c; bm = m; }
    }
    *best = b;
    return bm;
}
// WelsMdI4x4Fast's choice for one block (h264.wasm func 774 475164-476768; oracle h264o_i4_choose): c[m] = SAD +
// (m == predicted ? lambda : 4 lambda) for syntax mode m, uniform
DEV int i4_choose(const int *c, int ai, int *cost) {
    const int cnt = (int)((MD_I4_CNT4 >> (4 * ai)) & 15u);
    int best, m;
    if (cnt == 7 || cnt == 9) {
        const bool hb = c[1] < c[2];
        best = hb ? c[1] : c[2]; m = hb ? 1 : 2;
        if (c[0] < best) { best = c[0]; m = 0; }
        if (c[0] < c[1]) {
            if (cnt == 9) {
                if (c[5] < best) { best = c[5]; m = 5; }
                if (best > c[7]) { best = c[7]; m = 7; }
                if (!(c[0] <= c[7] && c[0] <= c[5])) {
                    if (c[5] < c[7]) { if (c[4] < best) { best = c[4]; m = 4; } }
                    else if (c[3] < best) { best = c[3]; m = 3; }
                }
            } else {
                if (c[4] < best) { best = c[4]; m = 4; }
                if (c[5] < best) { best = c[5]; m = 5; }
            }
        } else {
            if (c[6] < best) { best = c[6]; m = 6; }
            if (best > c[8]) { best = c[8]; m = 8; }
            if (!(c[6] >= c[1] && c[8] >= c[1])) {
                if (c[8] > c[6]) { if (c[4] < best) { best = c[4]; m = 4; } }
                else if (cnt == 9 && c[3] < best) { best = c[3]; m = 3; }
            }
        }
    } else {
        best = 0x7fffffff; m = 2;
        const uint32_t list = c_MD_I4_LIST4[ai];
        for (int i = 0; i < cnt; i++) {
            const int mm = (int)((list >> (4 * i)) & 15u);
            if (c[mm] < best) { best = c[mm]; m = mm; }
        }
    }
    *cost = best;
    return m;
}
// SAD of 16x16 mode m (wave-uniform) on the calling wave -> S.cand[20 + m] (lane = 4 * block + row)
DEV void i16_sad_mode(EncLds &S, const I16Ctx &k, int m) {
    const int lane = e_lane(), blk = lane >> 2, row = lane & 3;
    const int y = (blk >> 2) * 4 + row, x0 = (blk & 3) * 4;
    if (!i16_avail(k, m)) return;
    const uint32_t sv = *(const uint32_t *)&S.src[y * 16 + x0];
    int v = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) v += iabs((int)((sv >> (8 * j)) & 255) - i16_pred(S, k, m, x0 + j, y));
    const int sad = wave_sum(v);
    if (lane == 0) S.cand[20 + m] = sad;
}
// WelsMdI16x16's choice (func 313) from the mode SADs in S.cand[20..23] (after the barrier that published them): the
// first minimum of SAD + lambda x bits in md_i16_order(flags), uniform
DEV int i16_first_min(const EncLds &S, int lam, int flags, int *cost) {
    int c[4];
#pragma unroll
    for (int m = 0; m < 4; m++) c[m] = uni(S.cand[20 + m]);
    return md_first_min(md_i16_order(flags), c, lam, cost);
}
// I slices: wave w the SAD of mode w, then the choice. All waves call.
DEV int i16_decide_oh(EncLds &S, const I16Ctx &k, int lam, int flags, int *cost) {
    i16_sad_mode(S, k, uni(e_wave()));
    lds_barrier();
    return i16_first_min(S, lam, flags, cost);
}
// AnalysisVaaInfoIntra (func 854) of the source MB: sixteen 4x4 means (sum >> 4), sum of squares - (sum^2 >> 4);
// every wave, uniform
DEV int vaa_intra_var(const EncLds &S) {
    const int l = e_lane() & 15, bx = l & 3, by = l >> 2;
    int t = 0;
#pragma unroll
    for (int y = 0; y < 4; y++) {
        const uint32_t w = *(const uint32_t *)&S.src[(4 * by + y) * 16 + 4 * bx];
        t += (int)(w & 255) + (int)((w >> 8) & 255) + (int)((w >> 16) & 255) + (int)(w >> 24);
    }
    const int a = t >> 4;
    const uint32_t sum = (uint32_t)lane_read(group16_sum(a), 0), sq = (uint32_t)lane_read(group16_sum(a * a), 0);
    return (int)(sq - ((sum * sum) >> 4));
}

// ---------------------------------------------------------------- chroma intra prediction (8.3.4)
struct CCtx { int a[2], b[2], c[2], has_top, has_left; };
template <class LDS> DEV CCtx chroma_ctx(const LDS &S, int has_top, int has_left) {
    CCtx r;
    for (int pl = 0; pl < 2; pl++) {
        int H = 0, V = 0;
        for (int i = 0; i < 4; i++) {
            H += (i + 1) * (S.topc[pl][1 + 4 + i] - S.topc[pl][1 + 2 - i]);
            V += (i + 1) * (S.leftc[pl][4 + i] - (2 - i >= 0 ? S.leftc[pl][2 - i] : S.topc[pl][0]));
        }
        r.a[pl] = uni(16 * (S.leftc[pl][7] + S.topc[pl][8])); r.b[pl] = uni((34 * H + 32) >> 6); r.c[pl] = uni((34 * V + 32) >> 6);
    }
    r.has_top = has_top; r.has_left = has_left;
    return r;
}
template <class LDS> DEV int chroma_dc_blk(const LDS &S, const CCtx &k, int pl, int bx, int by) {
    int st = 0, sl = 0;
    for (int i = 0; i < 4; i++) { st += S.topc[pl][1 + 4 * bx + i]; sl += S.leftc[pl][4 * by + i]; }
    int t = k.has_top, l = k.has_left;
    if (bx == by) return (t && l) ? (st + sl + 4) >> 3 : l ? (sl + 2) >> 2 : t ? (st + 2) >> 2 : 128;
    if (bx == 1) return t ? (st + 2) >> 2 : l ? (sl + 2) >> 2 : 128;
    return l ? (sl + 2) >> 2 : t ? (st + 2) >> 2 : 128;
}
template <class LDS> DEV int chroma_pred(const LDS &S, const CCtx &k, int mode, int pl, int x, int y, int dcv) {
    int hv = mode == 1 ? S.leftc[pl][y] : S.topc[pl][1 + x];
    // plane parameters by select, not by a per-lane index into the arrays (that would put k in scratch)
    const int ka = pl ? k.a[1] : k.a[0], kb = pl ? k.b[1] : k.b[0], kc = pl ? k.c[1] : k.c[0];
    int pln = clip1((ka + kb * (x - 3) + kc * (y - 3) + 16) >> 5);
    return mode == 0 ? dcv : (mode <= 2 ? hv : pln);
}
DEV bool chroma_avail(const CCtx &k, int m) {
    return m == 0 || (m == 1 && k.has_left) || (m == 2 && k.has_top) || (m == 3 && k.has_top && k.has_left);
}
// mode decision on lanes 0..31 (mode*8 + plane*4 + block), then prediction fill; returns mode
// WelsMdIntraChroma (func 312): SAD(Cb) + SAD(Cr) + lambda x bits, the first minimum in md_chroma_order(flags)
__device__ __noinline__ int chroma_decide_fill(EncLds &S, int a0, int a1, int b0, int b1, int c0, int c1, int has_top, int has_left,
                                               int lam, int flags) {
    CCtx k;
    k.a[0] = uni(a0); k.a[1] = uni(a1); k.b[0] = uni(b0); k.b[1] = uni(b1); k.c[0] = uni(c0); k.c[1] = uni(c1);
    k.has_top = uni(has_top); k.has_left = uni(has_left);
    int lane = e_lane();  // decision: every wave (identical); fill: split over the workgroup
    int m = (lane >> 3) & 3, pl = (lane >> 2) & 1, blk = lane & 3, ox = (blk & 1) * 4, oy = (blk >> 1) * 4;
    int dcv = chroma_dc_blk(S, k, pl, blk & 1, blk >> 1);
    int d[16];
#pragma unroll
    for (int y = 0; y < 4; y++)
#pragma unroll
        for (int x = 0; x < 4; x++) d[4 * y + x] = S.srcc[pl][(oy + y) * 8 + ox + x] - chroma_pred(S, k, m, pl, ox + x, oy + y, dcv);
    int s = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) s += iabs(d[i]);
    s = group8_sum(s);
    int c[4];
#pragma unroll
    for (int mm = 0; mm < 4; mm++) c[mm] = lane_read(s, mm * 8);
    int bc;
    int best = uni(md_first_min(md_chroma_order(uni(flags)), c, uni(lam), &bc));
    for (int i = e_tid(); i < 128; i += ENC_THREADS) {
        int p2 = i >> 6, p = i & 63, x = p & 7, y = p >> 3;
        int dv = chroma_dc_blk(S, k, p2, x >> 2, y >> 2);
        S.predc[p2][p] = (uint8_t)chroma_pred(S, k, best, p2, x, y, dv);
    }
    lds_barrier();
    return best;
}
DEV int chroma_decide_fill(EncLds &S, const CCtx &k, int lam, int flags) {
    return uni(chroma_decide_fill(S, k.a[0], k.a[1], k.b[0], k.b[1], k.c[0], k.c[1], k.has_top, k.has_left, lam, flags));
}

// ---------------------------------------------------------------- motion vector prediction (8.4.1.3)
struct MvNb { int avail, ref, mx, my; };
DEV MvNb nb_from_payload(const uint32_t *p, int k, bool avail) {
    MvNb r;
    r.avail = avail;
    if (!avail) { r.ref = -1; r.mx = r.my = 0; return r; }
    r.ref = uni((int8_t)((p[8] >> (k < 2 ? 16 : 24)) & 255));
    r.mx = uni((int16_t)(p[12 + k] & 0xffff)); r.my = uni((int16_t)(p[12 + k] >> 16));
    return r;
}
DEV void mv_pred16(MvNb A, MvNb B, MvNb C, int out[2]) {
    if (!B.avail && !C.avail && A.avail) { B = A; C = A; }
    int n = (A.ref == 0) + (B.ref == 0) + (C.ref == 0);
    if (n == 1) {
        out[0] = A.ref == 0 ? A.mx : (B.ref == 0 ? B.mx : C.mx);  // field-wise: no MvNb copy through scratch
        out[1] = A.ref == 0 ? A.my : (B.ref == 0 ? B.my : C.my);
        return;
    }
    out[0] = median3(A.mx, B.mx, C.mx);
    out[1] = median3(A.my, B.my, C.my);
}
// integer-search start candidate n (0 mvp, 1 (0,0), 2 A, 3 B, 4 C; n per lane), integer-rounded and clipped
// to +-16; false when the neighbour is unavailable or not inter. Scalar arguments and selects: a member
// or array selected by a per-lane index would be copied through scratch.
DEV bool me_start_cand(int n, int p0, int p1, int amx, int amy, int bmx, int bmy, int cmx, int cmy, bool okA, bool okB, bool okC,
                       int &cx, int &cy) {
    const int mx = n == 2 ? amx : (n == 3 ? bmx : cmx), my = n == 2 ? amy : (n == 3 ? bmy : cmy);
    const bool ok = n == 2 ? okA : (n == 3 ? okB : okC);
    const int vx = n == 0 ? p0 : (n == 1 ? 0 : mx), vy = n == 0 ? p1 : (n == 1 ? 0 : my);
    cx = clip3(-16, 16, (vx + 2) >> 2); cy = clip3(-16, 16, (vy + 2) >> 2);
    return n < 2 || ok;
}
DEV int mvbits(int mx, int my, const int mvp[2]) { return se_len(mx - mvp[0]) + se_len(my - mvp[1]); }

// ---------------------------------------------------------------- motion search helpers
// 4 window bytes at absolute column gx of window row wr, plane p: two aligned dword reads + alignbyte
// (the ring wraps at dword granularity)
DEV uint32_t win4(const EncLds &S, int p, int wr, int gx) {
    const int sl = (gx + 24) & 63;
    const uint32_t *row = (const uint32_t *)&S.win[p][wr * WIN_STRIDE];
    return __builtin_amdgcn_alignbyte(row[((sl >> 2) + 1) & 15], row[sl >> 2], sl & 3);
}
// SAD of integer candidate (cx, cy) of this lane's 16-lane group: lane & 15 = MB row, 16 pixels per
// lane (v_sad_u8 x4), summed over the group with DPP. Every wave evaluates its own four groups: no
// barrier, and the waves reach identical (uniform) decisions.
DEV int sad16_row_group(const EncLds &S, int Y0, int X, int Y, int cx, int cy) {
    const int row = e_tid() & 15;
    const u32x4 sv = *(const u32x4 *)&S.src[row * 16];
    const int sl = (X + cx + 24) & 63, i0 = sl >> 2, sh = sl & 3;
    const uint32_t *rw = (const uint32_t *)&S.win[0][(Y + cy + row - Y0) * WIN_STRIDE];
    const uint32_t w0 = rw[i0], w1 = rw[(i0 + 1) & 15], w2 = rw[(i0 + 2) & 15], w3 = rw[(i0 + 3) & 15], w4 = rw[(i0 + 4) & 15];
    uint32_t acc = __builtin_amdgcn_sad_u8(sv.x, __builtin_amdgcn_alignbyte(w1, w0, sh), 0u);
    acc = __builtin_amdgcn_sad_u8(sv.y, __builtin_amdgcn_alignbyte(w2, w1, sh), acc);
    acc = __builtin_amdgcn_sad_u8(sv.z, __builtin_amdgcn_alignbyte(w3, w2, sh), acc);
    acc = __builtin_amdgcn_sad_u8(sv.w, __builtin_amdgcn_alignbyte(w4, w3, sh), acc);
    return group16_sum((int)acc);
}
// SATD of the whole MB predicted at the quarter-sample vector (mvx, mvy) (uniform in the wave):
// sum over the 16 4x4 blocks of (sum |H D H| + 1) >> 1 (DESIGN.md §3.5, same value as satd4 per
// block). Lane = 4 * block + row: one row of 4 differences per lane, horizontal Hadamard in
// registers, vertical Hadamard across the quad with DPP butterflies. Result uniform.
// N candidates at once (N uniform): the per-lane parts and the N reductions are independent chains
// the compiler interleaves, so a wave with two or three candidates pays little more than one.
template <int N> DEV void satd16_mv_n(const EncLds &S, int Y0, int X, int Y, const int *mvx, const int *mvy, int *out) {
    const int lane = e_tid() & 63, blk = lane >> 2, row = lane & 3;
    const int y = (blk >> 2) * 4 + row, x0 = (blk & 3) * 4;
    const uint32_t sv = *(const uint32_t *)&S.src[y * 16 + x0];
    const int s1 = (row & 1) ? -1 : 1, s2 = (row & 2) ? -1 : 1;
    int acc[N];
#pragma unroll
    for (int n = 0; n < N; n++) {
        const QSel q = qsel((mvy[n] & 3) * 4 + (mvx[n] & 3));
        const int gx = X + x0 + (mvx[n] >> 2), wr = Y + y + (mvy[n] >> 2) - Y0;
        const uint32_t pa = win4(S, q.p1, wr + q.dy1, gx + q.dx1), pb = win4(S, q.p2, wr + q.dy2, gx + q.dx2);
        const uint32_t pv = (pa | pb) - (((pa ^ pb) & 0xFEFEFEFEu) >> 1);  // bytewise (a + b + 1) >> 1
        const int d0 = (int)(sv & 255) - (int)(pv & 255), d1 = (int)((sv >> 8) & 255) - (int)((pv >> 8) & 255);
        const int d2 = (int)((sv >> 16) & 255) - (int)((pv >> 16) & 255), d3 = (int)(sv >> 24) - (int)(pv >> 24);
        const int a0 = d0 + d1, a1 = d0 - d1, a2 = d2 + d3, a3 = d2 - d3;
        int h0 = a0 + a2, h1 = a1 + a3, h2 = a0 - a2, h3 = a1 - a3;
        h0 = dpp<0xB1>(h0) + s1 * h0; h1 = dpp<0xB1>(h1) + s1 * h1; h2 = dpp<0xB1>(h2) + s1 * h2; h3 = dpp<0xB1>(h3) + s1 * h3;
        h0 = dpp<0x4E>(h0) + s2 * h0; h1 = dpp<0x4E>(h1) + s2 * h1; h2 = dpp<0x4E>(h2) + s2 * h2; h3 = dpp<0x4E>(h3) + s2 * h3;
        int v = iabs(h0) + iabs(h1) + iabs(h2) + iabs(h3);
        v += dpp<0xB1>(v);
        v += dpp<0x4E>(v);
        acc[n] = row == 0 ? (v + 1) >> 1 : 0;
    }
#pragma unroll
    for (int n = 0; n < N; n++) acc[n] = group16_sum(acc[n]);
#pragma unroll
    for (int n = 0; n < N; n++) out[n] = lane_read(acc[n], 0) + lane_read(acc[n], 16) + lane_read(acc[n], 32) + lane_read(acc[n], 48);
}
DEV int satd16_mv(const EncLds &S, int Y0, int X, int Y, int mvx, int mvy) {
    int r;
    satd16_mv_n<1>(S, Y0, X, Y, &mvx, &mvy, &r);
    return r;
}
// OpenH264's P_Skip judge (DESIGN.md §3.5; oracle pskip_residual_ok / sad_mb_pred / predict_sad_skip), per sample: the
// MB predicted at the skip vector (every lane stores the sample it used in S.pred / S.predc: a skipped MB's
// reconstruction) and its residual quantised at the MB's QP with inter rounding. Accumulated for the decision
// (pskip_take, after a barrier) in the MB's accumulator set J (EncLds::pj): J[1] the prediction's SAD, luma + chroma,
// J[3] its luma part (the intra test's inter cost); J[2] the luma blocks' single-coefficient costs; J[0] a rejection --
// a luma level above 1, a non-zero chroma DC level, a chroma level
// above 1 at any position (the DC position by the AC rule, as pfQuantizationFour4x4Max), or a chroma plane whose AC
// levels cost more than 6.
// Constants pinned to h264.wasm (tools/wasm_tables.py CODE_CONSTANTS pskip_*, TABLES single_ctr_run):
#define PSKIP_MV_MIN (-29)       // WelsMdPSkipEnc: (mv >> 2) + 16 * MB position below this: no skip (func 415, 234693)
#define PSKIP_MV_MAX_LOW 12      // ... or above (16 * MBs) | this (234709)
#define PSKIP_MAX_LEVEL 1        // a block with a larger |level| rejects (235268)
#define PSKIP_LUMA_CTR_MAX 5     // the MB's summed luma single-coefficient cost: at most this (235324)
#define PSKIP_CHROMA_CTR_MAX 6   // a chroma plane's: at most this (func 534, 281767)
#define PSKIP_SINGLE_CTR 0x56Bu  // WelsCalculateSingleCtr4x4's run table {3, 2, 2, 1, 1, 1, 0, ...} as 2-bit fields
// this lane's single-coefficient cost inside its 16-lane block: lane level lv at scan index zz; a non-zero level costs
// the table entry of the run of zeros below it (to the next non-zero level, or to the start)
DEV int single_ctr_lane(int lv, int zz) {
    const int m = group16_sum(lv != 0 ? 1 << zz : 0);  // the block's non-zero scan positions (distinct bits)
    const int lower = m & ((1 << zz) - 1);
    const int run = lower ? zz - 1 - (31 - __builtin_clz((unsigned)lower)) : zz;
    return lv != 0 ? (int)((PSKIP_SINGLE_CTR >> (2 * run)) & 3u) : 0;
}
// Exact all-zero pre-test (uniform thresholds, no decision changes): a coefficient of class k quantises to
// 0 iff |c| <= floor(65535 / MF_k) - FF_k (quant1), and the forward core transform bounds |c_uv| <= g_u g_v
// SAD with g = (1, 2, 1, 2) -- gain 1, 4, 2 for classes 0 (even/even), 1 (odd/odd), 2 (mixed). A 4x4 block
// whose SAD is at most the smallest T_k / gain_k therefore has only zero levels; the 2x2 chroma DC levels
// are bounded by the plane's SAD (|f| <= sum of the four blocks' |c_00|). Only a wave holding a block over
// its bound runs the transform and the quantiser.
// (class 0 also holds the AC positions (0,2), (2,0), (2,2): one bound serves luma blocks and chroma AC;
// negative: never proves zero)
DEV int zero_sad_bound(const QuantQP &q) {
    const int t0 = 65535 / q.mf0 - q.fp0, t1 = (65535 / q.mf1 - q.fp1) >> 2, t2 = (65535 / q.mf2 - q.fp2) >> 1;
    return min(t0, min(t1, t2));
}
// luma block lb of the skip prediction on this lane's 16-lane group: SAD, cost and rejection of the wave's blocks.
// Blocks whose SAD is under the all-zero bound (zero_sad_bound) skip the transform: their levels are all 0.
DEV void pskip_luma(EncLds &S, const Xf &X, const QuantQP &q, int Y0, int MX, int MY, int mvx, int mvy, int lb, int &lsad, int &ctr,
                    bool &rej) {
    const int pos = e_lane() & 15, lx = (lb & 3) * 4 + (pos & 3), ly = (lb >> 2) * 4 + (pos >> 2);
    const int pv = Wsample(S, Y0, MX + lx + (mvx >> 2), MY + ly + (mvy >> 2), mvx & 3, mvy & 3);
    S.pred[ly * 16 + lx] = (uint8_t)pv;
    const int dl = S.src[ly * 16 + lx] - pv;
    const int bs = group16_sum(iabs(dl));
    lsad += lane_read(bs, 0) + lane_read(bs, 16) + lane_read(bs, 32) + lane_read(bs, 48);
    if (__ballot(bs > zero_sad_bound(q)) != 0) {  // some block of this wave may have a level
        const int lv = quant1(xf_fwd(dl, X), qmf(q, X.cls), qff(q, X.cls, 0));
        rej = rej || iabs(lv) > PSKIP_MAX_LEVEL;
#ifndef H264MI_DIAG_NO_CTR  // timing diagnostic only: no single-coefficient costs (wrong skip decisions)
        ctr += wave_sum(single_ctr_lane(lv, X.zz));
#endif
    }
}
// chroma plane cp of the skip prediction on this wave (block lane >> 4): SAD, DC and level rejections, AC cost limit
DEV void pskip_chroma(EncLds &S, const Xf &X, const QuantQP &qc, int mbx, int mvx, int mvy, int cp, int &sad, bool &rej) {
    const int lane = e_lane(), pos = lane & 15, g = lane >> 4, cx = (g & 1) * 4 + (pos & 3), cy = (g >> 1) * 4 + (pos >> 2);
    const int pc = chroma_mc_sample(S, mbx, mvx, mvy, cp, cx, cy);
    S.predc[cp][cy * 8 + cx] = (uint8_t)pc;
    const int dc = S.srcc[cp][cy * 8 + cx] - pc;
    const int bs = group16_sum(iabs(dc));
    const int ps = lane_read(bs, 0) + lane_read(bs, 16) + lane_read(bs, 32) + lane_read(bs, 48);
    sad += ps;
    const int tdc = 65535 / (qc.mf0 >> 1) - 2 * qc.fp0;  // |2x2 DC| <= the plane's SAD
    if (__ballot(bs > zero_sad_bound(qc)) != 0 || ps > tdc) {
        const int t = xf_fwd(dc, X);
        const int lvc = quant1(t, qmf(qc, X.cls), qff(qc, X.cls, 0));
        const int a = lane_read(t, 0), b = lane_read(t, 16), e = lane_read(t, 32), f = lane_read(t, 48);
        const bool dcnz = quant_dc(a + b + e + f, qc.mf0, qc.fp0) != 0 || quant_dc(a - b + e - f, qc.mf0, qc.fp0) != 0 ||
                          quant_dc(a + b - e - f, qc.mf0, qc.fp0) != 0 || quant_dc(a - b - e + f, qc.mf0, qc.fp0) != 0;
#ifndef H264MI_DIAG_NO_CTR
        const int cctr = wave_sum(single_ctr_lane(X.zz > 0 ? lvc : 0, X.zz > 0 ? X.zz - 1 : 0));  // AC levels, AC scan
#else
        const int cctr = 0;
#endif
        rej = rej || iabs(lvc) > PSKIP_MAX_LEVEL || dcnz || cctr > PSKIP_CHROMA_CTR_MAX;
    }
}
DEV void pskip_publish(int *J, int lsad, int csad, int ctr, bool rej) {
    const int lane = e_lane();
    const bool r = __ballot(rej) != 0;
    if (lane == 0) {
        atomicAdd(&J[1], lsad + csad);
        atomicAdd(&J[3], lsad);
        if (ctr) atomicAdd(&J[2], ctr);
        if (r) atomicOr(&J[0], 1);
    }
}
// the judge on all four waves: luma blocks 4w .. 4w+3 on wave w, Cb on wave 0, Cr on wave 1 (the schedule for MBs
// predicted to be skipped: the left MB was; the integer search and the intra SATDs then run only if it rejects)
DEV void pskip_judge_4w(EncLds &S, int *J, const Xf &X, int qp, int Y0, int MX, int MY, int mbx, int mvx, int mvy) {
    const int w = e_wave(), g = e_lane() >> 4;
    const QuantQP q = make_qqp(qp), qc = make_qqp(c_CHROMA_QP[qp]);
    int lsad = 0, csad = 0, ctr = 0;
    bool rej = false;
    pskip_luma(S, X, q, Y0, MX, MY, mvx, mvy, 4 * w + g, lsad, ctr, rej);
    if (w < 2) pskip_chroma(S, X, qc, mbx, mvx, mvy, w, csad, rej);
    pskip_publish(J, lsad, csad, ctr, rej);
}
// the judge on waves 1..3 while wave 0 runs the integer search (MBs predicted not to be skipped): luma blocks
// 4(w-1) .. 4(w-1)+3 on wave w, then blocks 12..15 on wave 1, Cb on wave 2 and Cr on wave 3
DEV void pskip_judge_3w(EncLds &S, int *J, const Xf &X, int qp, int Y0, int MX, int MY, int mbx, int mvx, int mvy) {
    const int w = e_wave(), g = e_lane() >> 4;
    const QuantQP q = make_qqp(qp), qc = make_qqp(c_CHROMA_QP[qp]);
    int lsad = 0, csad = 0, ctr = 0;
    bool rej = false;
    pskip_luma(S, X, q, Y0, MX, MY, mvx, mvy, 4 * (w - 1) + g, lsad, ctr, rej);
    if (w == 1) pskip_luma(S, X, q, Y0, MX, MY, mvx, mvy, 12 + g, lsad, ctr, rej);
    else pskip_chroma(S, X, qc, mbx, mvx, mvy, w - 2, csad, rej);
    pskip_publish(J, lsad, csad, ctr, rej);
}
// luma + chroma SAD of S.pred / S.predc against the source, whole workgroup (the double check's skip SAD); judged: the
// judge ran at this vector and J[1] already holds it
DEV int mb_pred_sad(EncLds &S, int *J, bool judged) {
    if (judged) return uni(J[1]);
    const int tid = e_tid();
    int v = iabs((int)S.src[tid] - (int)S.pred[tid]);
    if (tid < 128) v += iabs((int)S.srcc[tid >> 6][tid & 63] - (int)S.predc[tid >> 6][tid & 63]);
    v = wave_sum(v);
    if ((tid & 63) == 0) atomicAdd(&J[1], v);
    lds_barrier();
    return uni(J[1]);
}
// luma prediction of the MB at the quarter-sample vector (mvx,mvy), whole workgroup
DEV void fill_pred_mv(EncLds &S, int Y0, int X, int Y, int mvx, int mvy) {
    const int i = e_tid();  // ENC_THREADS == 256: one sample each
    S.pred[i] = (uint8_t)Wsample(S, Y0, X + (i & 15) + (mvx >> 2), Y + (i >> 4) + (mvy >> 2), mvx & 3, mvy & 3);
}

// ---------------------------------------------------------------- the kernel
#define CAND(k) uni(S.cand[k])
// P slices, the first wait of an MB: lanes 0..15 poll the granules of (mbx, mby-1), lanes 16..31 those of
// (mbx+1, mby-1) (if it exists); only the decision granules 8 (type / QP / reference) and 12..15 (vectors)
DEV bool p_need1(int lane, bool has_next) {
    const int k = lane & 15;
    return (lane < 16 || (lane < 32 && has_next)) && (k == 8 || k >= 12);
}
// Workgroups take tickets in the order they start: tickets [0, S*mbh) are MB-row encoders, tickets
// [S*mbh, 2*S*mbh) deblocking rows (wave 0; waves 1 and 2 run the CAVLC of the row) that trail them, fed by the 128 granules per MB the
// encoder rows publish (deblock.inc). A deblocking row only waits on rows with lower tickets, which
// have started and stay resident, so any dispatch order and any residency limit make progress.
// Occupancy target (waves per SIMD): 4 (128 VGPRs, 4 encoder workgroups per CU). The waves are
// latency-bound (barriers, LDS and DPP chains), so residency pays: 2 -> 4 per SIMD took the 240-step
// bench 2920 -> 3030 frames/s with 77 VGPRs spilled, and 3760 once the spills were gone (e_tid: the
// lane-derived addresses are recomputed at their uses instead of living across the MB loop; 235 -> 136
// VGPRs unconstrained, 1 spill at 128). 5 per SIMD (96 VGPRs, 37 spills) measured slower (3650).
// tools/ab_bench.sh, tools/enc_var.sh. 0 = no target.
// Two builds of the kernel (LEAN): the occupancy-target build above, and an unconstrained one
// (lane ids read once, registers as the compiler likes) for launches whose rows fit the CUs at two
// workgroups each -- there residency buys nothing and the lean build's recomputation costs 5-10 %
// (1 stream 2.30 vs 2.44 ms per frame, 720p x 8 streams 3.50 vs 3.72 ms; runtime_enc.inc enc_frame).
// A/B switches of round 5's latency changes (tools/ab_tl.sh, profiles/round5/ab_*.txt): the prefetch commit
// at the next MB's start (slower); one barrier closing each MB; the row above's pixel granules loaded at the
// MB's start (neutral, off); the search phase's layout (0: top samples + I16 context behind a barrier, modes
// w - 1 on waves 1..3; 1: the same without the barrier, balanced modes -- 2-3 % faster rows; 2: each wave
// derives them after its test / search -- no better than 1)
#ifndef H264MI_ENC_REC_WAVE
#define H264MI_ENC_REC_WAVE 0  // the wave that stores the MB record (3: measured slower, row 0 +3 %)
#endif
#ifndef H264MI_ENC_LATE_COMMIT
#define H264MI_ENC_LATE_COMMIT 0
#endif
#ifndef H264MI_ENC_ONEBAR
#define H264MI_ENC_ONEBAR 1
#endif
#ifndef H264MI_ENC_XF_LDS
#define H264MI_ENC_XF_LDS 1
#endif
#ifndef H264MI_ENC_ST2PF
#define H264MI_ENC_ST2PF 0
#endif
#ifndef H264MI_ENC_PH1
#define H264MI_ENC_PH1 1
#endif
#ifndef H264MI_ENC_LATE_PF
#define H264MI_ENC_LATE_PF 0
#endif
#ifndef H264MI_ENC_WPE
#define H264MI_ENC_WPE 4
#endif
template <bool LEAN>
__global__ __launch_bounds__(ENC_THREADS)
__attribute__((amdgpu_waves_per_eu(LEAN && H264MI_ENC_WPE > 0 ? H264MI_ENC_WPE : 1, LEAN && H264MI_ENC_WPE > 0 ? H264MI_ENC_WPE : 8)))
void enc_mb_kernel(EncLaunch a) {
    struct DbkCavlcLds { DbkLds d; CavlcTabs T; CavlcWaveLds w[2]; };
    static_assert(sizeof(DbkCavlcLds) <= sizeof(EncLds), "the deblocking workgroup fits the encoder's LDS");
    __shared__ union { EncLds e; DbkCavlcLds k; } SH;
    EncLds &S = SH.e;
    __shared__ int s_ticket;
    const int wv = threadIdx.x >> 6;
    // tid / lane re-read at every use (e_tid): hoisted out of the MB loop, everything derived from them
    // stays live across the whole MB and spills at the occupancy target
#define tid (LEAN ? e_tid() : (int)threadIdx.x)
#define lane (tid & 63)
    // XCD-partitioned tickets (a.xq = 8, S % 8 == 0): workgroup blockIdx.x runs on XCD blockIdx.x % 8
    // (round-robin dispatch), takes its ticket from that XCD's queue, and the queue's tickets cover
    // streams q, q + 8, ... only -- every row of a stream runs on one XCD and its reference windows
    // meet in that XCD's L2. Each queue gets exactly 2 * (S / 8) * mbh workgroups, and a row still
    // waits only on lower tickets of its own queue, so the forward-progress argument holds per queue
    // whatever the actual placement.
    const int xq = a.xq, xqi = xq ? (int)(blockIdx.x & 7) : 0, Sq = xq ? a.S >> 3 : a.S;
    if (tid == 0) s_ticket = (int)atomicAdd(a.ticket + (xq ? 8 + xqi : 0), 1u);
    lds_barrier();
    // ticket -> (encoder or deblocking row, MB row, stream): blocks of Sq tickets; with dlag = D > 0 the
    // order is encoder rows 0..D-1, then deblocking row j and encoder row j + D alternately, then the
    // last D deblocking rows -- every row still waits only on rows with lower tickets
    // With a.sgrp = G < Sq the queue's streams are taken G at a time: the 2 G mbh tickets of streams 0..G-1 (in the
    // order above), then those of the next G. A stream's rows then run close together -- row r + 1 a few MBs behind
    // row r instead of ~mbw / (rows in flight per stream) -- so the reference windows it shares with the row above
    // are still in the XCD's L2 (round 6: at 128 streams, 16 per queue, 39 % of enc_mb_kernel's L2 requests missed,
    // 14 % at 32). Rows wait only on rows of their own stream, all in the same group, so the order stays safe.
    const int t = uni(s_ticket), lagD = a.dlag;
    int tb, tsq;
    if (a.sgrp > 0 && a.sgrp < Sq) {
        const int per = 2 * a.mbh * a.sgrp, g = t / per, tt = t - g * per, gs = min(a.sgrp, Sq - g * a.sgrp);
        tb = tt / gs;
        tsq = g * a.sgrp + (tt - tb * gs);
    } else {
        tb = t / Sq;
        tsq = t - tb * Sq;
    }
    const int ts = xq ? tsq * 8 + xqi : tsq;
    // diagnostics (H264MI_ENC_TL): this ticket's start and end on the GPU's constant 100 MHz clock
    const int tl_slot = xq ? xqi * 2 * Sq * a.mbh + t : t;
    if (a.tl && threadIdx.x == 0) a.tl[2 * tl_slot] = __builtin_amdgcn_s_memrealtime();
    auto tl_end = [&]() {  // each wave: the ticket's end is its last wave's
        if (a.tl && (threadIdx.x & 63) == 0)
            atomicMax((unsigned long long *)&a.tl[2 * tl_slot + 1], (unsigned long long)__builtin_amdgcn_s_memrealtime());
    };
    bool is_dbk;
    int trow;
    if (a.gomr > 0) {  // exact GOM rate control: GOM-major, each GOM's encoder rows then its deblocking / CAVLC rows
        const int R = a.gomr, k = min(tb / (2 * R), (a.mbh - 1) / R), rows_k = min(R, a.mbh - k * R), ph = tb - 2 * R * k;
        is_dbk = ph >= rows_k;
        trow = k * R + (is_dbk ? ph - rows_k : ph);
    } else if (lagD <= 0 || lagD >= a.mbh) { is_dbk = tb >= a.mbh; trow = is_dbk ? tb - a.mbh : tb; }
    else if (tb < lagD) { is_dbk = false; trow = tb; }
    else {
        const int k = tb - lagD, m = 2 * (a.mbh - lagD);
        if (k < m) { is_dbk = !(k & 1); trow = is_dbk ? (k >> 1) : lagD + (k >> 1); }
        else { is_dbk = true; trow = (a.mbh - lagD) + (k - m); }
    }
    if (is_dbk) {  // deblocking row (wave 0) and the CAVLC of its macroblocks (waves 1, 2)
        const int dby = trow, dsi = ts;
        if (wv == 3 || dby >= a.mbh) return;
        if (uni(cst(a.desc)[dsi].st->cur_skip)) return;  // frame skipped by the rate control
        if (wv == 0) {
            CONSTANT const DbkDesc &DD = cst(a.dbk)[dsi];
            const DbkLaunch dl{a.mbw, a.mbh, a.S, a.dbk, nullptr, a.dprof};
            CONSTANT const EncDesc &DE = cst(a.desc)[dsi];
            // the filter crosses slice edges (disable_deblocking_filter_idc 0); only the QPY entering a row knows them
            const int nsl = uni(DE.st->cur_slices);
            deblock_row(SH.k.d, dl, DD, dby, DbkSrcGranules{gbl((const uint64_t *)DD.src_gran), a.mbw, dby, (uint32_t)uni((int)*DD.epoch),
                                                            gbl((const uint64_t *)DE.rowq), uni(DE.st->cur_qp),
                                                            slice_row_first(a.mbh, nsl, dby), dby > 0 && slice_row_first(a.mbh, nsl, dby - 1)});
        } else {
            CONSTANT const EncDesc &D = cst(a.desc)[dsi];
            cavlc_row(SH.k.T, SH.k.w[wv - 1], D, a.mbw, a.mbh, dby, wv - 1, 2, (uint32_t)uni((int)D.st->epoch), &D.st->err, a.gomr > 0);
        }
        tl_end();
        return;
    }
    const int mby = trow, sidx = ts;
    // encoder progress for other streams' kernels (h264mi_enc_rows_counter): MB-row workgroups started since the
    // encoder's creation, monotonic (ticket[32], never reset) -- a launch k has started all its rows once it
    // reaches (k + 1) S mbh. The decoder's reconstruction can be gated on it (h264mi_dec_set_recon_gate).
    if (threadIdx.x == 0) __hip_atomic_fetch_add(a.ticket + 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the encoder rows are the launch's critical path; the deblocking rows that share their SIMDs trail them
    // (diagnostic, H264MI_ENC_PRIO): 1..3 every encoder row at that priority; 4 / 5 only the picture's first and
    // last MB rows -- the heavy ones on the launch's critical path (their P_Skip predictors fail) -- at 3 / 2
    if (a.prio == 1) __builtin_amdgcn_s_setprio(1);
    else if (a.prio == 2) __builtin_amdgcn_s_setprio(2);
    else if (a.prio == 3) __builtin_amdgcn_s_setprio(3);
    else if (a.prio == 4 && (trow == 0 || trow == a.mbh - 1)) __builtin_amdgcn_s_setprio(3);
    else if (a.prio == 5 && (trow == 0 || trow == a.mbh - 1)) __builtin_amdgcn_s_setprio(2);
    CONSTANT const EncDesc &D = cst(a.desc)[sidx];  // scalar loads, fields in SGPRs
    EncState *st = D.st;
    const uint32_t epoch = (uint32_t)uni((int)st->epoch);
    const int mbw = a.mbw, cw = mbw * 16, ch = a.mbh * 16, w = a.w, h = a.h;
    if (uni(st->cur_skip)) {  // frame skipped by the rate control: the reference stays the picture
        for (int pl = 0; pl < 3; pl++) {
            const int pw = pl ? cw / 2 : cw, rows = pl ? 8 : 16, n4 = pw / 4;
            GLOBAL const uint32_t *rs = (GLOBAL const uint32_t *)(gbl(D.ref[pl]) + (size_t)mby * rows * pw);
            GLOBAL uint32_t *rd = (GLOBAL uint32_t *)(gbl(D.dbk[pl]) + (size_t)mby * rows * pw);
            for (int i = tid; i < rows * n4; i += ENC_THREADS) rd[i] = rs[i];
        }
        GLOBAL const int32_t *ks = gbl(D.sksad_ref);  // and so does the P_Skip judge's memory of it
        GLOBAL int32_t *kd = gbl(D.sksad_cur);
        for (int i = tid; i < mbw; i += ENC_THREADS) kd[mby * mbw + i] = ks[mby * mbw + i];
        if (mby == 0 && tid == 0) kd[mbw * a.mbh] = ks[mbw * a.mbh];
        return;
    }
    // MB-row (GOM) QP of this row (DESIGN.md §3.6): every MB is decided and quantised at it; an MB
    // carrying mb_qp_delta moves the running QP there, any other MB's QPY is the running QP -- the QP
    // entering the row for the MBs before the row's first carrier (record flag 0x80, resolved by the
    // deblocking row and the CAVLC from rowq), the row QP after it
    const int idr = uni(st->cur_idr), slice_qp = uni(st->cur_qp);
    // slices of whole MB rows (DESIGN.md §3.7): nothing above a slice's first row is available (7.4.3) -- no wait on
    // the row above, no neighbour from it -- and that row is entered at the slice QP. Uniform, decided once per row;
    // the picture's row 0 is the single-slice case of it.
    const int sl_row0 = slice_first_row(a.mbh, uni(st->cur_slices), slice_of_row(a.mbh, uni(st->cur_slices), mby));
    // an IDR is coded at the frame QP (OpenH264 turns the GOM QP off for I slices in RC_BITRATE_MODE, h264.wasm
    // func 1226 766730-766775); a P row at the frame QP + its planned offset inside the frame's window
    int32_t *abort_word = &st->err;
    int qp;
    if (a.gomr > 0 && !idr) {  // OpenH264's GOM rule (exact mode): the GOM's QP from the bits of every MB before it
        if (wv == 0) {
            const int g = gom_row_qp(D, st, mby, mbw, a.gomr, epoch, abort_word);
            if (lane == 0) S.gom_qp = g < 0 ? slice_qp : g;  // a failed wait: the frame is aborting anyway
        }
        lds_barrier();
        qp = uni(S.gom_qp);
    } else {
        qp = idr ? slice_qp : clip3(uni(st->rc.min_frame_qp), uni(st->rc.max_frame_qp), slice_qp + uni(gbl(D.rowqp)[mby]));
    }
    GLOBAL uint64_t *rowq = gbl(D.rowq);
    bool row_carried = false;
    const QuantQP q = make_qqp(qp);
    const int qpc = c_CHROMA_QP[qp];
    const QuantQP qc = make_qqp(qpc);
    const int lam = c_LAMBDA[qp];
#if H264MI_ENC_XF_LDS
    // the transforms' lane constants (10 dwords per lane) live in LDS, read where used: held in registers across
    // the MB loop they were 10 VGPRs of a kernel that spills at its 128-VGPR occupancy target
    if (tid < 16) S.xft[tid] = xf_consts(tid);
#define XF (S.xft[e_tid() & 15])
#else
    const Xf XF = xf_consts(tid & 15);  // lane constants of the 4x4 transforms
#endif
    const int Y0 = mby * 16 - 24, Y = mby * 16;
    // global-address-space views of everything the wavefront touches (no flat ops: see h264mi_dev.h)
    GLOBAL const uint8_t *srcY = gbl(a.src_base) + (size_t)sidx * a.src_stride, *srcU = srcY + (size_t)w * h, *srcV = srcU + (size_t)(w / 2) * (h / 2);
    // The predicate `above` rides on a value that is live across the MB loop anyway -- the row above's granules, null
    // when there is no such row -- so it costs no register of its own in a kernel that spills at its occupancy target
    // (see XF above). WARNING: grow_prev is null in a slice's first row: every use of it must stay behind `above`
    // (an unguarded grow_prev + ... there is a GPU fault, not a harmless read of row 0 as it once was).
    GLOBAL uint64_t *const grow_prev = mby > sl_row0 ? gbl(D.gran) + (size_t)(mby - 1) * mbw * H264MI_GRANULES_PER_MB : nullptr;
#define above (grow_prev != nullptr)
    GLOBAL uint64_t *grow = gbl(D.gran) + (size_t)mby * mbw * H264MI_GRANULES_PER_MB;
    GLOBAL uint64_t *egr = gbl(D.egran);
    GLOBAL uint32_t *info32 = gbl((uint32_t *)D.info);
    GLOBAL MbCoef *coefg = gbl(D.coef);
    if (tid == 0) S.abort_flag = 0;
    int L_ref = -1, L_mvx = 0, L_mvy = 0;  // left MB: reference index, vector (MV prediction, 8.4.1.3)
    bool L_skip = false;                   // left MB was P_Skip (the P_Skip judge; the next MB's schedule prediction)
    int L_sksad = -1;                      // left MB's skip SAD (PredictSadSkip)
    bool i4_dirty = false;                 // the last MB was an Intra4x4 MB of a P slice: S.i4 back to 2 (DC) first
    // the P_Skip judge's memory of the reference picture (DESIGN.md §3.5): is it a P picture, and per MB the skip SAD
    // of a skipped MB (-1: not skipped), read one MB ahead; this frame's goes to D.sksad_cur with the outputs
    // (the row's words go to LDS at the row start: a global load inside the MB loop would be waited for behind the
    // previous MB's write-through output stores -- vmcnt counts loads and stores in order)
    GLOBAL const int32_t *skref = gbl(D.sksad_ref) + (size_t)mby * mbw;
    const bool ref_p = !idr && uni(gbl(D.sksad_ref)[mbw * a.mbh]) != 0;
    if (ref_p)
        for (int i = tid; i < mbw; i += ENC_THREADS) S.refsk[i] = skref[i];
    if (mby == 0 && tid == 0) gbl(D.sksad_cur)[mbw * a.mbh] = idr ? 0 : 1;
    uint32_t L_i4 = 0;                     // left MB: Intra4x4 modes of its right column (bytes, by block row)
    // section timer (H264MI_ENC_PROF): 1 wait row above, 2 loads+context, 3 P_Skip test, 4 integer ME,
    // 5 sub-pel, 6 intra alternative, 7 P16x16 residual, 8 I4 search, 9 I-MB residual, 10 outputs
    // 16..19 each wave's own busy time in the outputs section up to its barrier, 20..23 each wave's time from
    // the outputs section's start to the end of its prefetch commit (H264MI_ENC_LATE_COMMIT: from the MB's start,
    // wave 0's poll included); P MBs whose test runs beside
    // the integer search, from the start of that phase: 24..27 wave w's P_Skip test (wave 0: its start
    // candidates), 28..31 its first I16 mode (wave 0: the diamond), 32..35 its last task (-> a.prof[16 + k];
    // none of these is part of the total)
    __shared__ uint64_t s_prof[40];  // 36..39: outputs section, wave w's time to its first store group's end
#if defined(H264MI_ENC_PROF_BUILD) || defined(H264MI_ENC_PROF_DETAIL)
    // section counters (H264MI_ENC_PROF=1) only in a profiling build loaded through H264MI_LIB
    // (-DH264MI_ENC_PROF_BUILD, or the detail build): in the default build their clock reads kept SGPRs live
    // across the MB loop (195 -> 171 spilled SGPRs, which live in VGPR lanes)
    const bool prof = a.prof != nullptr && (a.prof_row < 0 || a.prof_row == mby);
#else
    constexpr bool prof = false;
#endif
    uint64_t t_prev = 0;
    if (prof) { if (tid < 40) s_prof[tid] = 0; t_prev = clock64(); }
    // slots 16..35 only in a -DH264MI_ENC_PROF_DETAIL build (H264MI_LIB=...): their clock reads and atomics cost
    // the default build SGPR spills (178 -> 216) and ~5 % on row 0 even with profiling off
    auto stamp = [&](int k, uint64_t t0) {
#ifdef H264MI_ENC_PROF_DETAIL
        if (prof && (threadIdx.x & 63) == 0) atomicAdd((unsigned long long *)&s_prof[k], (unsigned long long)(clock64() - t0));
#endif
    };
    auto lap = [&](int k) { if (prof) { uint64_t tt = clock64(); if (tid == 0) s_prof[k] += tt - t_prev; t_prev = tt; } };
#ifdef H264MI_ENC_FINE  // finer split (slots 11..15): pred fills, first SADs, the two SATD passes, P16 pred
    auto lapf = lap;
#else
    auto lapf = [](int) {};
#endif
    lds_barrier();

    // ---- reference windows and source, one MB ahead (enc_mb.inc: window layout)
    // pfw: luma window strip of plane tid >> 6, window row tid & 63 (16 columns);
    // pfa: wave 0 -> chroma window strip (plane lane >> 5, row lane & 31, 8 columns, .xy);
    //      wave 1 lanes 0..15 -> source luma row, lanes 16..31 -> source chroma row (.xy)
    const int ps = D.ps, psc = D.psc;
    // the lane's window-row addresses (recomputing them at each use frees four VGPRs but measured 3 % slower
    // beside the decoder, profiles/round5/ab_bisect_bench.txt)
    GLOBAL const uint8_t *plw = gbl(D.pl[tid >> 6]) + (ptrdiff_t)(Y0 + (tid & 63)) * ps;
    GLOBAL const uint8_t *plcw = gbl(D.plc[(tid >> 5) & 1]) + (ptrdiff_t)(mby * 8 - 12 + (tid & 31)) * psc;
    // aligned whole-row source loads, prefetched one MB ahead (uniform per row); rows past the picture's
    // bottom (the cropped last MB row: 1080p codes 1088 rows) read the last picture row -- the vertical edge
    // replication of load_src_bytes. That row used to load byte by byte, unprefetched: 1.6 ms of a 3.9 ms
    // 32-stream launch instead of ~0.7 ms, on the launch's critical path (profiles/round5/timeline_s32.txt)
    const bool vsrc = a.src_vec != 0;
    u32x4 pfw = {0, 0, 0, 0}, pfa = {0, 0, 0, 0};
    auto issue_prefetch = [&](int nx) {
        if (!idr) {
            pfw = *(GLOBAL const u32x4 *)(plw + 16 * nx + 24);
            if (wv == 0) pfa.xy = *(GLOBAL const u32x2 *)(plcw + 8 * nx + 12);
        }
        if (vsrc && wv == 1) {
            if (lane < 16) pfa = *(GLOBAL const u32x4 *)(srcY + (size_t)min(Y + lane, h - 1) * w + 16 * nx);
            else if (lane < 32) {
                const int pl = (lane - 16) >> 3, r = (lane - 16) & 7;
                pfa.xy = *(GLOBAL const u32x2 *)((pl ? srcV : srcU) + (size_t)min(mby * 8 + r, h / 2 - 1) * (w / 2) + 8 * nx);
            }
        }
    };
    auto commit_prefetch = [&](int nx) {
        if (!idr) {
            win_put4(&S.win[tid >> 6][(tid & 63) * WIN_STRIDE + ((16 * nx + 48) & 63)], pfw);
            if (wv == 0) win_put2(&S.winc[lane >> 5][(lane & 31) * WINC_STRIDE + ((8 * nx + 24) & 31)], pfa.xy);
        }
        if (vsrc && wv == 1) {
            if (lane < 16) *(u32x4 *)&S.src[lane * 16] = pfa;
            else if (lane < 32) *(u32x2 *)&S.srcc[(lane - 16) >> 3][((lane - 16) & 7) * 8] = pfa.xy;
        }
    };
    auto load_src_bytes = [&](int mbx) {  // edge-replicated source MB (picture edges, odd sizes)
        const int X = mbx * 16, i = tid;
        int x = min(X + (i & 15), w - 1), y = min(Y + (i >> 4), h - 1);
        S.src[i] = srcY[(size_t)y * w + x];
        if (tid < 128) {
            int pl = tid >> 6, p = tid & 63;
            x = min(mbx * 8 + (p & 7), w / 2 - 1); y = min(mby * 8 + (p >> 3), h / 2 - 1);
            S.srcc[pl][p] = (pl ? srcV : srcU)[(size_t)y * (w / 2) + x];
        }
    };
    if (!idr) {  // initial window: luma columns [-24, 40), chroma [-12, 20)
#pragma unroll
        for (int k = 0; k < 4; k++)
            win_put4(&S.win[tid >> 6][(tid & 63) * WIN_STRIDE + 16 * k], *(GLOBAL const u32x4 *)(plw - 24 + 16 * k));
        if (wv == 0) {
#pragma unroll
            for (int k = 0; k < 4; k++)
                win_put2(&S.winc[lane >> 5][(lane & 31) * WINC_STRIDE + 8 * k], *(GLOBAL const u32x2 *)(plcw - 12 + 8 * k));
        }
    }
    load_src_bytes(0);
    if (tid < 16) { S.left[tid] = 0; S.leftc[tid >> 3][tid & 7] = 0; S.i4[tid] = 2; }
    if (tid < 8) S.pj[tid >> 2][tid & 3] = 0;  // the P_Skip judge's accumulators, both MB parities
    static_assert(sizeof(I4Table) == 9 * 16 * 8, "I4Tap is 8 bytes");
    for (int i = tid; i < 9 * 16 * 2; i += ENC_THREADS) ((uint32_t *)S.i4t)[i] = ((const uint32_t *)&c_I4)[i];
    lds_barrier();

    int mbx_cur = 0;
    // P slices: the decision granules of this MB for the row below (type | qp | ref, vectors), as soon
    // as the decision is made; the rest of the record follows with the outputs
    // (granule 13 carries the MB's skip SAD instead of a vector: the MV prediction reads 12 and 15)
    auto publish_decision = [&](int ty, int mx, int my, int sk) {
        if (wv == 1 && (lane == 8 || (lane >= 12 && lane < 16))) {
            const bool in = ty == MI_I4 || ty == MI_I16;
            const uint32_t v = lane == 8 ? (uint32_t)ty | ((uint32_t)qp << 8) | (in ? 0xffff0000u : 0u)
                                         : (lane == 13 ? (uint32_t)sk : (uint32_t)(uint16_t)mx | ((uint32_t)(uint16_t)my << 16));
            gran_store(grow + (size_t)mbx_cur * 16 + lane, epoch, v);
        }
    };
    uint64_t top_pf = 0;  // wave 0, P slices: the next MB's row-above granules, loaded one MB ahead
    // wave 0, P slices (H264MI_ENC_ST2PF): the row above's pixel granules of an MB (stage 2: the intra test of an MB the
    // P_Skip judge does not take, or takes without bKeepSkip), loaded with the previous MB's outputs, ahead of its stores
    // -- loaded at stage 2 they waited for the previous MB's write-through stores (vmcnt counts loads and stores in
    // order): one hand-off round trip (~2k cycles) on each such MB; checked, and polled again if stale, at use
    // at use: those already published are taken at the MB's first wait (step 1), which covers their load; only a set
    // with a stale granule is loaded again by the stage-2 poll (a wait there is vmcnt(0): the MB's window prefetch and
    // the previous MB's write-through stores)
    uint64_t st2_pf = 0;
    bool st2_stale = true;  // wave 0: some stage-2 granule of this MB was not yet published at step 1
    auto st2_need = [&](int nx) { return lane < 8 || lane == 9 || (nx > 0 && (lane == 19 || lane == 21 || lane == 23)); };
    auto st2_load = [&](int nx) -> uint64_t {
        return st2_need(nx) ? __hip_atomic_load(grow_prev + (size_t)(lane < 16 ? nx : nx - 1) * 16 + (lane & 15), __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT)
                            : 0;
    };
    int pend127 = -1;     // wave 2: the MB whose granule 127 is still to go out (after its coefficient stores)
    for (int mbx = 0; mbx < mbw; mbx++) {
        const int X = mbx * 16;
        mbx_cur = mbx;
        // ---- 1. wait for the row above. I slices: the whole record of (mbx+1, mby-1) (Intra4x4 uses its
        // bottom pixels), plus (0, mby-1) at row start. P slices: the decision granules (8: type/ref,
        // 12..15: vectors) of (mbx, mby-1) and (mbx+1, mby-1), which the row above publishes right after its
        // decision, before its residual coding; prefetched at the previous MB. The P_Skip test needs nothing
        // else; only an MB it rejects waits for the row above's pixels (its intra alternative), after it.
        // (H264MI_ENC_LATE_COMMIT, measured slower and off) the window strips and source prefetched at the
        // previous MB committed to LDS here instead of in that MB's outputs section: a wave's wait on its
        // prefetch registers also waits for every memory operation it issued before them (vmcnt counts loads
        // and stores, in order), and here that includes the output stores it has just issued -- one write-through
        // round trip per MB, on the critical path wherever no poll hides it (row 0: 1.35-1.40 -> 1.46-1.56 ms
        // per row, profiles/round5/ab_commit.txt). In the outputs section the commit precedes the MB's stores.
        auto commit_here = [&]() {
            if (H264MI_ENC_LATE_COMMIT && mbx > 0) {
                commit_prefetch(mbx);
                stamp(20 + wv, t_prev);
            }
        };
        if (wv != 0 || !above) commit_here();
        if (above) {  // wave 0 polls, the workgroup follows through LDS
            if (wv == 0) {
                bool ok = true;
                if (idr) {
                    uint32_t v;
                    if (mbx == 0) {
                        ok = gran_wait(grow_prev, 16, epoch, &v, abort_word);
                        if (ok && lane < 16) S.gp[0][lane] = v;
                    }
                    if (ok && mbx + 1 < mbw) {
                        ok = gran_wait(grow_prev + (size_t)(mbx + 1) * 16, 16, epoch, &v, abort_word);
                        if (ok && lane < 16) S.gp[(mbx + 1) % 3][lane] = v;
                    }
                } else {
                    const bool need = p_need1(lane, mbx + 1 < mbw);
#if H264MI_ENC_ST2PF
                    // later MBs': loaded with the previous MB's outputs. Issued before this poll's wait, which then
                    // covers it (vmcnt is in order): stage 2 then tests it with no wait of its own
                    if (mbx == 0) st2_pf = st2_load(0);
#endif
                    if (mbx == 0) top_pf = need ? __hip_atomic_load(grow_prev + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
                    ok = gran_poll(grow_prev + (size_t)mbx * 16 + lane, need, epoch, top_pf, abort_word);
                    if (ok && need) S.gp[(mbx + (lane >> 4)) % 3][lane & 15] = (uint32_t)top_pf;
#if H264MI_ENC_ST2PF
                    {  // the stage-2 granules already published
                        const bool need2 = st2_need(mbx), fresh = (uint32_t)(st2_pf >> 32) == epoch;
                        if (ok && need2 && fresh) S.gp[(lane < 16 ? mbx : mbx - 1) % 3][lane & 15] = (uint32_t)st2_pf;
                        st2_stale = __ballot(need2 && !fresh) != 0;
                    }
#endif
                }
                if (!ok && lane == 0) S.abort_flag = 1;
                commit_here();
            }
            lds_barrier();
            if (S.abort_flag) return;
        }
        lap(mbx == 0 ? 0 : 1);  // profile: the row-start wait (wavefront ramp) apart from the steady-state waits
        // ---- 2. next MB's window strips and source into registers; this MB's source if not prefetched
        const int ref_sk = ref_p ? uni(S.refsk[mbx]) : -1;  // the co-located MB of the reference picture: its skip SAD, -1 if not skipped
        // (H264MI_ENC_LATE_PF, A/B only: P slices issue it after their decision (1) or just before the P_Skip judge (2) --
        // loads in flight across the P path's start make the compiler wait for them, and so for the previous MB's output
        // stores, before reusing their registers; both only moved that wait, profiles/round6/eprof/encprof_s128_{i,j}.txt)
        if (mbx + 1 < mbw && (idr || !H264MI_ENC_LATE_PF)) issue_prefetch(mbx + 1);
        if (!vsrc && mbx > 0) load_src_bytes(mbx);
        // ---- 3. neighbour pixel context from the granule ring and the left MB
        const bool has_top = above, has_left = mbx > 0, has_tr = above && mbx + 1 < mbw, has_tl = has_top && has_left;
        const int nbf = (int)has_left | ((int)has_top << 1) | ((int)has_tl << 2) | ((int)has_tr << 3);  // OpenH264's MB flags
        const uint32_t *PB = S.gp[mbx % 3], *PC = S.gp[(mbx + 1) % 3], *PD = S.gp[(mbx + 2) % 3];
        // top row (+ top-left, top-right) luma and chroma samples from the granules. all_waves: every wave
        // writes the same values (P slices: each wave then reads its own writes, no barrier needed before
        // the reads -- the previous MB's readers all ended at its barriers); else wave 0 only
        // One lane-addressed dword read of the granule ring per lane (lanes 0..20 luma: 0 top-left, 1..16 top,
        // 17..20 top-right; lanes 32..49 chroma: plane (l - 32) / 9, 0 top-left, 1..8 top) -- no per-lane if-chain
        // of LDS reads.
        auto fill_top = [&](bool all_waves, bool tr) {
            const int i = all_waves ? lane : tid;
            const bool luma = i < 21, chroma = i >= 32 && i < 50;
            const int pl = (i - 32) / 9, k = (i - 32) - 9 * pl;
            // granule dword g of the ring slot of MB mbx - 1 + (g >> 4): 0.. (mbx, row above), 16.. (mbx + 1), 32.. (mbx - 1)
            const int g = luma ? (i == 0 ? 2 * 16 + 3 : (i <= 16 ? (i - 1) >> 2 : 16 + ((i - 17) >> 2)))
                               : (chroma ? (k == 0 ? 2 * 16 + 5 + 2 * pl : 4 + 2 * pl + ((k - 1) >> 2)) : 0);
            const uint32_t w = S.gp[(mbx + (g >> 4)) % 3][g & 15];
            const int sh = luma ? (i == 0 ? 24 : 8 * ((i - 1) & 3)) : (k == 0 ? 24 : 8 * ((k - 1) & 3));
            const bool av = luma ? (i == 0 ? has_tl : (i <= 16 ? has_top : (has_tr && tr))) : (k == 0 ? has_tl : has_top);  // top-right: I4 only
            const uint8_t v = av ? (uint8_t)(w >> sh) : (uint8_t)0;
            if (luma) S.top[i] = v;
            if (chroma) S.topc[pl][k] = v;
        };
        // P slices: the row above's pixel granules, polled by wave 0 (the workgroup follows through LDS). tr = false:
        // the rest of (mbx, mby-1)'s record -- granules 0..7 (bottom samples), 9 (bottom Intra4x4 modes) -- and the
        // top-left samples of (mbx-1, mby-1) (granules 3, 5, 7), published with their outputs; tr = true: the top-right
        // samples, granules 0..3 of (mbx+1, mby-1) (an intra MB's Intra4x4 search). false: the frame is aborting.
        auto poll_above = [&](bool tr) -> bool {
            if (!above || (tr && !has_tr)) return true;
            if (wv == 0 && (tr || !H264MI_ENC_ST2PF || st2_stale)) {  // (ST2PF: published ones were taken at step 1)
#ifndef H264MI_DIAG_NO_G9  // timing diagnostic only: granule 9 not polled (wrong Intra4x4 mode prediction in P slices)
                const bool need = tr ? lane < 4 : (lane < 8 || lane == 9 || (mbx > 0 && (lane == 19 || lane == 21 || lane == 23)));
#else
                const bool need = tr ? lane < 4 : (lane < 8 || (mbx > 0 && (lane == 19 || lane == 21 || lane == 23)));
#endif
                const int nb = tr ? mbx + 1 : (lane < 16 ? mbx : mbx - 1);
                GLOBAL uint64_t *g = grow_prev + (size_t)nb * 16 + (lane & 15);
                uint64_t x = need ? __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
                const bool ok = gran_poll(g, need, epoch, x, abort_word);
                if (ok && need) S.gp[nb % 3][lane & 15] = (uint32_t)x;
                if (!ok && lane == 0) S.abort_flag = 1;
            }
            lds_barrier();
            return !S.abort_flag;
        };
        // P slices write nothing here: the left samples are zeroed at the row start, S.i4 stays 2 (reset after an
        // Intra4x4 MB), the P_Skip judge's words are cleared at the previous MB's end and the prefetched source is
        // committed there -- so no barrier (only the byte-wise source loads and the I slices' top samples need one)
        if (idr) fill_top(false, true);
        if (idr || i4_dirty) {
            if (tid < 16) S.i4[tid] = 2;
        }
        if (idr || !vsrc || i4_dirty) lds_barrier();
        i4_dirty = false;

        int type = MI_I16, cbp = 0, i16mode = 0, cmode = 0, mvx = 0, mvy = 0, mvdx = 0, mvdy = 0;
        int cur_sk = -1;  // this MB's skip SAD if it is skipped (the judge's memory)
        int *J = S.pj[mbx & 1];  // this MB's P_Skip judge accumulators
        lap(2);
        // every MB of an I slice, and the MBs of a P slice that WelsMdFirstIntraMode codes intra, go through the intra
        // coding below with their I16x16 context, mode and cost
        bool do_intra = idr;
        I16Ctx k16;
        int m16 = 0, c16 = 0x7fffffff;
        if (idr) {
            // ================= I slice: I16x16 vs I4x4 (DESIGN.md §3.3)
            // (DESIGN.md §3.3: OpenH264's WelsMdIntraMb -- I16x16 by SAD, Intra4x4 only above the VAA variance
            // threshold, WelsMdI4x4Fast per block, the search stopped once the blocks cost the I16x16 cost)
            k16 = i16_ctx(S, has_top, has_left);
            m16 = i16_decide_oh(S, k16, lam, nbf, &c16);
        } else {
            // ================= P slice (DESIGN.md §3.5)
#ifdef H264MI_ISA_MARK  // ISA inspection only: the P path's start in the assembly
            asm volatile(";;MARK_PSTART" ::: "memory");
#endif
            MvNb A, B, C;
            A.avail = has_left;
            if (has_left) { A.ref = L_ref; A.mx = L_mvx; A.my = L_mvy; } else { A.ref = -1; A.mx = A.my = 0; }
            B = nb_from_payload(PB, 0, has_top);
            C = has_tr ? nb_from_payload(PC, 0, true) : nb_from_payload(PD, 3, has_tl);
            int mvp[2], skmv[2] = {0, 0};
            mv_pred16(A, B, C, mvp);
            if (has_left && has_top && !(A.ref == 0 && A.mx == 0 && A.my == 0) && !(B.ref == 0 && B.mx == 0 && B.my == 0)) {
                skmv[0] = mvp[0]; skmv[1] = mvp[1];
            }
            // 1. OpenH264's P_Skip judge (DESIGN.md §3.5; WelsMdInterMb func 746, WelsMdPSkipEnc func 415): tried only
            // when the left, top, top-left or top-right MB was skipped or (P reference picture) the co-located MB was,
            // and the skip vector is in range; taken when the prediction's SAD is 0, below the neighbours' predicted
            // skip SAD (PredictSadSkip func 331) or below the co-located MB's, else when the residual passes. For MBs it
            // rejects (or does not try), the integer search and the intra 16x16 SATDs. Two schedules, chosen per MB
            // from a prediction (the decisions are the same): predicted skip (the left MB was skipped; the MB above at
            // a row start) -- the judge on all four waves first, which needs only the row above's decision granules,
            // the rest only if it rejects; predicted coded -- the row above's pixels first, then the judge on waves
            // 1..3 beside the search on wave 0.
            const bool skA = has_left && L_skip, skB = has_top && (uni((int)PB[8]) & 255) == MI_PSKIP;
            const bool skC = has_tr && (uni((int)PC[8]) & 255) == MI_PSKIP, skD = has_tl && (uni((int)PD[8]) & 255) == MI_PSKIP;
            const bool ref_skip = ref_p && ref_sk >= 0;
            const int sx = (skmv[0] >> 2) + 16 * mbx, sy = (skmv[1] >> 2) + 16 * mby;
#ifndef H264MI_DIAG_ALWAYS_TRY  // timing diagnostic only: the judge run for every MB (wrong decisions)
            const bool try_skip = (skA || skB || skC || skD || ref_skip) && sx >= PSKIP_MV_MIN && sx <= ((16 * mbw) | PSKIP_MV_MAX_LOW) &&
                                  sy >= PSKIP_MV_MIN && sy <= ((16 * a.mbh) | PSKIP_MV_MAX_LOW);
#else
            const bool try_skip = true;
#endif
            auto pskip_take = [&]() -> bool {  // after the barrier that ends the judge
                const int sA = skA ? L_sksad : 0, sB = skB ? uni((int)PB[13]) : 0;
                const bool skCC = has_tr ? skC : skD;
                const int sC = skCC ? uni((int)(has_tr ? PC[13] : PD[13])) : 0;
                const int f = (int)skA | ((int)skB << 1) | ((int)skCC << 2);
                const int pred = (!has_top && !has_tl && has_left) ? sA : (f == 1 ? sA : (f == 2 ? sB : (f == 4 ? sC : median3(sA, sB, sC))));
                const int tsad = uni(J[1]);
                const bool res_ok = uni(J[0]) == 0 && uni(J[2]) <= PSKIP_LUMA_CTR_MAX;
                return tsad == 0 || tsad < pred || (ref_skip && tsad < ref_sk) || res_ok;
            };
            const bool pred_skip = has_left ? L_skip : skB;
            const bool beside = try_skip && !pred_skip;  // the judge runs on waves 1..3 beside the search
            bool skip_taken = false;
            if (H264MI_ENC_LATE_PF == 2 && mbx + 1 < mbw) issue_prefetch(mbx + 1);
#ifdef H264MI_ISA_MARK
            asm volatile(";;MARK_JUDGE" ::: "memory");
#endif
            if (try_skip && pred_skip) {
                pskip_judge_4w(S, J, XF, qp, Y0, X, Y, mbx, skmv[0], skmv[1]);
                lds_barrier();
                skip_taken = pskip_take();
            }
            const bool me_ran = !skip_taken;  // the integer search and the I16x16 SADs run (the judge beside, or none)
            if (!skip_taken) {
                // the row above's pixels for the intra alternative
                if (!poll_above(false)) return;
                // each wave fills the top samples and derives the I16 context itself, after its test or search (no
                // barrier: fill_top(true)); they are needed by the I16 modes and, after the join, by every wave
#if H264MI_ENC_PH1 == 0
                fill_top(false, false);
                lds_barrier();
                k16 = i16_ctx(S, has_top, has_left);
#elif H264MI_ENC_PH1 == 1
                fill_top(true, false);
                k16 = i16_ctx(S, has_top, has_left);
#endif
#ifdef H264MI_ENC_PROF_DETAIL
                const uint64_t t_ph = prof ? clock64() : 0;
#else
                const uint64_t t_ph = 0;
#endif
                // 2. integer search on wave 0 (DESIGN.md §3.5) beside the intra 16x16 SADs on waves 1..3 (and, for a
                // predicted-coded MB, the P_Skip test): start candidates {mvp, (0,0), A, B, C} (integer-rounded,
                // clipped to +-16; A/B/C only when available and inter), iterated small diamond, range +-16. Each
                // step's candidates are evaluated on the wave's four 16-lane groups and picked with one packed-key
                // minimum (cost << k | order): the decisions of the one-at-a-time sequential search (first
                // minimal candidate wins; strict improvement to move). After the barrier, if the best cost is
                // still above CROSS_THR, all four waves run the cross search.
                if (wv != 0) {
                    // the I16 modes: beside the test (a luma pass ~1.0k cycles, a luma + chroma pass ~3.0k, a mode
                    // ~1.1k, the search 2.5-3.3k; profiles/round5/encprof_rows_s32_row{0,67}.txt) wave 1 takes modes 1 and 0,
                    // wave 3 mode 3, the search's wave mode 2 (DC, always available); after a failed 4-wave test,
                    // wave w takes mode w - 1 and wave 1 mode 3 as well
#if H264MI_ENC_PH1 == 0
                    if (beside) pskip_judge_3w(S, J, XF, qp, Y0, X, Y, mbx, skmv[0], skmv[1]);
                    i16_sad_mode(S, k16, uni(wv - 1));
                    if (wv == (beside ? 3 : 1)) i16_sad_mode(S, k16, 3);
#else
                    if (beside) {
                        pskip_judge_3w(S, J, XF, qp, Y0, X, Y, mbx, skmv[0], skmv[1]);
                        stamp(24 + wv, t_ph);
#if H264MI_ENC_PH1 == 2
                        fill_top(true, false);
                        k16 = i16_ctx(S, has_top, has_left);
#endif
                        if (wv == 1) i16_sad_mode(S, k16, 1);
                        stamp(28 + wv, t_ph);
                        if (wv == 1) i16_sad_mode(S, k16, 0);
                        else if (wv == 3) i16_sad_mode(S, k16, 3);
                        stamp(32 + wv, t_ph);
                    } else {
#if H264MI_ENC_PH1 == 2
                        fill_top(true, false);
                        k16 = i16_ctx(S, has_top, has_left);
#endif
                        i16_sad_mode(S, k16, uni(wv - 1));
                        if (wv == 1) i16_sad_mode(S, k16, 3);
                    }
#endif
                } else {
                    const int grp = (tid >> 4) & 3;
                    int bx, by, bc;
                    {
                        // candidate n: 0 mvp, 1 (0,0), 2 A, 3 B, 4 C
                        // the neighbours' fields as plain scalars, the candidate picked by selects (n is per lane):
                        // selecting a whole MvNb, or capturing A/B/C by reference, copies them through scratch
                        const bool okA = A.avail & (A.ref == 0), okB = B.avail & (B.ref == 0), okC = C.avail & (C.ref == 0);
                        const int amx = A.mx, amy = A.my, bmx = B.mx, bmy = B.my, cmx = C.mx, cmy = C.my, p0 = mvp[0], p1 = mvp[1];
                        auto cand_xy = [&](int n, int &cx, int &cy) -> bool {
                            return me_start_cand(n, p0, p1, amx, amy, bmx, bmy, cmx, cmy, okA, okB, okC, cx, cy);
                        };
                        int cx, cy;
                        bool av = cand_xy(grp, cx, cy);
                        int cost = sad16_row_group(S, Y0, X, Y, cx, cy) + lam * mvbits(4 * cx, 4 * cy, mvp);
                        int k = wave_min(av ? (cost << 3) | grp : 0x7fffffff);
                        if (uni((int)okC)) {  // candidate 4 on group 0's lanes
                            av = cand_xy(4, cx, cy) && grp == 0;
                            cost = sad16_row_group(S, Y0, X, Y, cx, cy) + lam * mvbits(4 * cx, 4 * cy, mvp);
                            k = min(k, wave_min(av ? (cost << 3) | 4 : 0x7fffffff));
                        }
                        bc = k >> 3;
                        cand_xy(k & 7, bx, by);
                    }
                    if (beside) stamp(24, t_ph);
                    lapf(12);
                    for (int it = 0; it < 32; it++) {
                        // diamond order (0,-1), (-1,0), (1,0), (0,1); out-of-range points never chosen
                        const int cx = bx + (grp == 1 ? -1 : (grp == 2 ? 1 : 0)), cy = by + (grp == 0 ? -1 : (grp == 3 ? 1 : 0));
                        const int sad = sad16_row_group(S, Y0, X, Y, cx, cy);
                        const bool ok = cx >= -16 && cx <= 16 && cy >= -16 && cy <= 16;
                        const int k = wave_min(ok ? ((sad + lam * mvbits(4 * cx, 4 * cy, mvp)) << 2) | grp : 0x7fffffff);
                        if (k == 0x7fffffff || (k >> 2) >= bc) break;
                        bc = k >> 2;
                        bx += (k & 3) == 1 ? -1 : ((k & 3) == 2 ? 1 : 0);
                        by += (k & 3) == 0 ? -1 : ((k & 3) == 3 ? 1 : 0);
                    }
                    if (lane == 0) { S.cand[17] = bx; S.cand[18] = by; S.cand[19] = bc; }
#if H264MI_ENC_PH1 == 2
                    fill_top(true, false);
                    k16 = i16_ctx(S, has_top, has_left);
#endif
#if H264MI_ENC_PH1 != 0
                    if (beside) {
                        stamp(28, t_ph);
                        i16_sad_mode(S, k16, 2);
                        stamp(32, t_ph);
                    }
#endif
                }
#ifndef H264MI_ENC_FINE  // profile: each wave's own busy time in this section (slots 11 + wave), before the join
                if (prof && lane == 0) atomicAdd((unsigned long long *)&s_prof[11 + wv], (unsigned long long)(clock64() - t_prev));
#endif
                lds_barrier();
                if (beside) skip_taken = pskip_take();
            }
            if (H264MI_ENC_LATE_PF == 1 && mbx + 1 < mbw) issue_prefetch(mbx + 1);
            lap(3);
            // 3. WelsMdFirstIntraMode (func 747): the MB is coded intra when its I16x16 cost (SAD + lambda x mode bits, the
            // first minimum in the pinned order, §3.3) is below the inter cost -- a taken skip's luma SAD (bMdUsingSad, the
            // wrapper's complexity 0) unless the left, top and top-right MBs were skipped (bKeepSkip); else the integer
            // search's cost (this project's search, after its cross search), before the sub-pel refinement
#ifndef H264MI_DIAG_NO_SKIP_INTRA
            if (skip_taken && !(skA && skB && skC)) {
#else  // timing diagnostic only (wrong decisions): no intra test for a taken skip
            if (false) {
#endif
                if (!me_ran) {  // the skip was taken before the row above's pixels: fetch them, then the four I16x16 SADs
                    if (!poll_above(false)) return;
                    fill_top(true, false);
                    k16 = i16_ctx(S, has_top, has_left);
                    i16_sad_mode(S, k16, uni(wv));
                    lds_barrier();
                }
                m16 = i16_first_min(S, lam, nbf, &c16);
                do_intra = c16 < uni(J[3]);
            }
            if (skip_taken && !do_intra) {  // P_Skip: the reconstruction is the prediction
                type = MI_PSKIP; mvx = skmv[0]; mvy = skmv[1]; cbp = 0;
                cur_sk = uni(J[1]);
                publish_decision(type, mvx, mvy, cur_sk);
                // no copy to S.rec: the outputs read a skipped MB's reconstruction from S.pred / S.predc, which
                // the test completed before the barrier that published its answer
            } else if (!skip_taken) {
                int bx = uni(S.cand[17]), by = uni(S.cand[18]), bcf = uni(S.cand[19]);
                if (uni(S.cand[19]) > ENC_CROSS_THR) {
                    // cross search: the horizontal line through the best point (x = -16..16, order 0..32),
                    // then the vertical line (y = -16..16, order 33..65); packed key (cost << 7) | order, strict
                    // improvement. The best point itself sits on both lines and costs exactly bc, so it can never
                    // be strictly better: it is left out, and the other 64 candidates fill four passes of the
                    // 16 groups (j = 16 pass + group; wave = (j >> 2) & 3) instead of five -- same decisions
                    const int bc = uni(S.cand[19]);
                    int kl = 0x7fffffff;  // per-lane minimum over the passes (each 16-lane group's key is uniform in it),
                                          // one wave minimum after the last pass instead of one per pass
#pragma unroll 1
                    for (int pass = 0; pass < 4; pass++) {
                        const int j = pass * 16 + ((tid >> 4) & 15), hz = j < 32, i = hz ? j : j - 32;
                        const int t = i - 16 + (i - 16 >= (hz ? bx : by) ? 1 : 0);  // -16..16 without the best point's coordinate
                        const int cx = hz ? t : bx, cy = hz ? by : t, k = hz ? t + 16 : t + 49;
                        const int sad = sad16_row_group(S, Y0, X, Y, cx, cy);
                        kl = min(kl, ((sad + lam * mvbits(4 * cx, 4 * cy, mvp)) << 7) | k);
                    }
                    const int kmin = wave_min(kl);
                    if (lane == 0) S.cand[24 + wv] = kmin;
                    lds_barrier();
                    const int km = min(min(uni(S.cand[24]), uni(S.cand[25])), min(uni(S.cand[26]), uni(S.cand[27])));
                    if ((km >> 7) < bc) {
                        const int k = km & 127;
                        if (k < 33) bx = k - 16; else by = k - 49;
                        bcf = km >> 7;
                    }
                }
                lap(4);
                m16 = i16_first_min(S, lam, nbf, &c16);
                do_intra = c16 < bcf;
              if (!do_intra) {
                // 3. half then quarter refinement by SATD (wave w takes candidates w, w+4, w+8), then a
                // packed-key minimum over the candidates in lanes (order: current best first)
                const int wv4 = uni(tid >> 6);
                {
                    int mx[3], my[3], cv[3];
#pragma unroll
                    for (int n = 0; n < 3; n++) {
                        const int k = wv4 + 4 * n - 1;
                        mx[n] = 4 * bx + (k < 0 ? 0 : 2 * sub_dx(k & 7)); my[n] = 4 * by + (k < 0 ? 0 : 2 * sub_dy(k & 7));
                    }
                    if (wv4 == 0) {  // candidates 0 (the integer position), 4, 8
                        satd16_mv_n<3>(S, Y0, X, Y, mx, my, cv);
                        if (lane == 0) { S.cand[0] = cv[0]; S.cand[4] = cv[1]; S.cand[8] = cv[2]; }
                    } else {
                        satd16_mv_n<2>(S, Y0, X, Y, mx, my, cv);
                        if (lane == 0) { S.cand[wv4] = cv[0]; S.cand[wv4 + 4] = cv[1]; }
                    }
                }
                lds_barrier();
                lapf(13);
                int bdx, bdy, sc;
                {
                    const int k = lane - 1, ddx = lane == 0 ? 0 : 2 * sub_dx(k & 7), ddy = lane == 0 ? 0 : 2 * sub_dy(k & 7);
                    const int key = lane < 9 ? ((S.cand[lane] + lam * mvbits(4 * bx + ddx, 4 * by + ddy, mvp)) << 4) | lane : 0x7fffffff;
                    const int m = wave_min(key), o = m & 15;
                    sc = m >> 4;
                    bdx = o == 0 ? 0 : 2 * sub_dx(o - 1); bdy = o == 0 ? 0 : 2 * sub_dy(o - 1);
                }
                {
                    int mx[2], my[2], cv[2];
#pragma unroll
                    for (int n = 0; n < 2; n++) { mx[n] = 4 * bx + bdx + sub_dx(wv4 + 4 * n); my[n] = 4 * by + bdy + sub_dy(wv4 + 4 * n); }
                    satd16_mv_n<2>(S, Y0, X, Y, mx, my, cv);
                    if (lane == 0) { S.cand[9 + wv4] = cv[0]; S.cand[13 + wv4] = cv[1]; }
                }
                lds_barrier();
                lapf(14);
                {
                    const int ddx = bdx + sub_dx(lane & 7), ddy = bdy + sub_dy(lane & 7);
                    const int key = lane < 8 ? ((S.cand[9 + lane] + lam * mvbits(4 * bx + ddx, 4 * by + ddy, mvp)) << 4) | (lane + 1)
                                             : (lane == 8 ? sc << 4 : 0x7fffffff);
                    const int m = wave_min(key), o = m & 15;
                    sc = m >> 4;
                    if (o > 0) { bdx += sub_dx(o - 1); bdy += sub_dy(o - 1); }
                }
                lap(5);
                {
                    // 5. P16x16 at the refined vector
                    type = MI_P16x16;
                    mvx = 4 * bx + bdx; mvy = 4 * by + bdy;
                    const bool at_skmv = mvx == skmv[0] && mvy == skmv[1];  // its type waits for the double check
                    if (!at_skmv) publish_decision(type, mvx, mvy, -1);
                    mvdx = mvx - mvp[0]; mvdy = mvy - mvp[1];
                    fill_pred_mv(S, Y0, X, Y, mvx, mvy);
                    chroma_mc(S, mbx, mby, mvx, mvy);
                    lapf(15);
                    cbp = code_residual_nodc(S, XF, qp, 0, 1, true);
                    if (at_skmv) {  // 6. WelsMdInterDoubleCheckPskip (func 399): no coded residual at the skip vector: P_Skip
                        if (cbp == 0) { type = MI_PSKIP; cur_sk = mb_pred_sad(S, J, try_skip); }
                        publish_decision(type, mvx, mvy, cur_sk);
                    }
                }
                lap(7);
              }
            }
        }
        if (do_intra) {
            // ================= intra MB: Intra4x4 (VAA-gated WelsMdI4x4Fast search, func 774) or I16x16 (DESIGN.md §3.3)
            // a P slice's intra MB: the row below learns "intra, no vector, no skip SAD" now (what its decisions read from
            // granule 8; Intra4x4 or I16x16 comes with the record and granule 9, after the search)
            if (!idr) publish_decision(MI_I16, 0, 0, -1);
            int cost4 = 0;
            bool won = vaa_intra_var(S) > 149;  // WelsMdIntraFinePartitionVaa (func 774, 474996)
            if (!idr && won) {  // the Intra4x4 search in a P slice: the row above's bottom modes (granule 9) are in, its
                // top-right samples (granules 0..3 of (mbx+1, mby-1)) are fetched now
                if (!poll_above(true)) return;
                fill_top(false, true);
                lds_barrier();
            }
            for (int blk = 0; won && blk < 16; blk++) {
                const int ras = (blk & 8) | ((blk & 2) << 1) | ((blk & 4) >> 1) | (blk & 1), bx = ras & 3, by = ras >> 2, ox = bx * 4, oy = by * 4;
                const bool bt = by > 0 || has_top, bl = bx > 0 || has_left;
                bool btr;
                if (by == 0) btr = bx < 3 ? has_top : has_tr;
                else btr = (bx < 3) && ras != 5 && ras != 13;  // top-right block already coded (6.4.11.4)
                if (tid < 13) {  // block context (single writer)
                    int v = 0;
                    if (lane == 0) {
                        if (bt && bl) v = (bx > 0 && by > 0) ? S.rec[(oy - 1) * 16 + ox - 1] : (by > 0 ? S.left[oy - 1] : S.top[ox]);
                    } else if (lane <= 8) {
                        int i = lane - 1;
                        if (bt) {
                            int ii = (i >= 4 && !btr) ? 3 : i;
                            v = by > 0 ? S.rec[(oy - 1) * 16 + ox + ii] : S.top[1 + ox + ii];
                        }
                    } else {
                        int i = lane - 9;
                        if (bl) v = bx > 0 ? S.rec[(oy + i) * 16 + ox - 1] : S.left[oy + i];
                    }
                    S.n4[lane] = (uint8_t)v;
                }
                lds_barrier();
                const int ma = uni(bx > 0 ? S.i4[ras - 1] : (has_left ? (int)(int8_t)(L_i4 >> (8 * by)) : -1));
                const int mb = uni(by > 0 ? S.i4[ras - 4] : (has_top ? (int)(int8_t)((PB[9] >> (8 * bx)) & 255) : -1));
                const int pm = (ma < 0 || mb < 0) ? 2 : min(ma, mb);
                const int s4t = S.n4[1] + S.n4[2] + S.n4[3] + S.n4[4], s4l = S.n4[9] + S.n4[10] + S.n4[11] + S.n4[12];
                const int dcv = (bt && bl) ? (s4t + s4l + 4) >> 3 : bl ? (s4l + 2) >> 2 : bt ? (s4t + 2) >> 2 : 128;
                // the nine modes' SADs, lane-parallel: pass k puts mode 4k + (lane >> 4) on each 16-lane row (lane & 15
                // = raster position), row sums by DPP reductions; the modes a block may not use are never read
                int cm[9];
                {
                    const int p = lane & 15, g = lane >> 4;
                    const int sv = S.src[(oy + (p >> 2)) * 16 + ox + (p & 3)];
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        const int m = 4 * k + g;
                        const int pv = m == 2 ? dcv : i4_tap_eval(S.i4t[m < 9 ? m : 8][p], S.n4);
                        const int sad = group16_sum(iabs(sv - pv));
#pragma unroll
                        for (int gg = 0; gg < 4; gg++)
                            if (4 * k + gg < 9) cm[4 * k + gg] = lane_read(sad, 16 * gg) + ((4 * k + gg) == pm ? lam : lam << 2);
                    }
                }
                int bcost;
                const int best = i4_choose(cm, (int)((c_MD_I4_IDX4[nbf] >> (4 * blk)) & 15u), &bcost);
                cost4 += bcost;
                if (cost4 >= c16) { won = false; break; }
                if (wv == 0) {  // code the 4x4 block (intra rounding, all 16 coefficients): lane p = raster
                    // position p of the block (lanes 16.. repeat the block), lane-per-coefficient DPP transforms
                    const int p = lane & 15, o = (oy + (p >> 2)) * 16 + ox + (p & 3);
                    const int pv = best == 2 ? dcv : i4_tap_eval(S.i4t[best][p], S.n4);
                    const int t = xf_fwd(S.src[o] - pv, XF);
                    const int lv = quant1(t, qmf(q, XF.cls), qff(q, XF.cls, 1));
                    const int n = (int)popc(__ballot(lv != 0) & 0xffffu);
                    const int r = (xf_inv((lv * (XF.cls == 0 ? q.v0 : (XF.cls == 1 ? q.v1 : q.v2))) << q.q6, XF) + 32) >> 6;
                    if (lane < 16) {
                        S.rec[o] = (uint8_t)clip1(pv + r);
                        S.lvl[ras][XF.zz] = (int16_t)lv;
                    }
                    if (lane == 0) { S.nnz[ras] = n; S.i4[ras] = (int8_t)best; }
                }
                lds_barrier();
            }
            lap(8);
            won = won && cost4 + 24 * lam < c16;
            const CCtx kc = chroma_ctx(S, has_top, has_left);
            if (won) {
                type = MI_I4;
                cmode = chroma_decide_fill(S, kc, lam, nbf);
                cbp = code_residual_nodc(S, XF, qp, 1, 0, true);
            } else {
                type = MI_I16; i16mode = m16;
                if (tid < 16) S.i4[tid] = 2;
                i16_fill_pred(S, k16, m16);
                cmode = chroma_decide_fill(S, kc, lam, nbf);
                cbp = code_residual(S, XF, qp, 1, 1, 1);
            }
            if (!idr) i4_dirty = type == MI_I4;
            lap(9);
        }
        // ---- 4. the window is no longer read (every path ended at a barrier): slide it, stage the next
        // source MB; then the outputs, one wave each: MB record (wave 0), hand-off granules (wave 1),
        // coefficient blocks (wave 2), unfiltered reconstruction (wave 3)
        if (!H264MI_ENC_LATE_COMMIT && mbx + 1 < mbw) {
            commit_prefetch(mbx + 1);
            stamp(20 + wv, t_prev);
        }
        if (!idr && wv == 0 && above && mbx + 1 < mbw) {  // the next MB's row-above granules (checked, polled if stale, there)
            const bool need = p_need1(lane, mbx + 2 < mbw);
#if H264MI_ENC_ST2PF
            st2_pf = st2_load(mbx + 1);  // first: the next MB's stage-1 wait (on top_pf) then covers it
#endif
            top_pf = need ? __hip_atomic_load(grow_prev + (size_t)(mbx + 1) * 16 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        }
        const int mbi = mby * mbw + mbx;
        const bool intra = type == MI_I4 || type == MI_I16, skip = type == MI_PSKIP;
        const uint32_t mvw = (uint32_t)(uint16_t)mvx | ((uint32_t)(uint16_t)mvy << 16), refw = intra ? 0xffffffffu : 0u;
        // the record and hand-off dwords that live in LDS, gathered with one dword read per lane at a lane-selected
        // address (the per-lane if-chains with byte reads compiled to a serial run of LDS round trips, ~1.5k cycles
        // of the outputs section per wave, profiles/round5/encprof_outputs_detail.txt)
        constexpr int O_I4 = offsetof(EncLds, i4) / 4, O_NZ = offsetof(EncLds, nnz) / 4;
        // this MB's reconstruction: S.rec / S.recc, or for a skipped MB its prediction
        const int O_REC = skip ? (int)(offsetof(EncLds, pred) / 4) : (int)(offsetof(EncLds, rec) / 4);
        const int O_RECC = skip ? (int)(offsetof(EncLds, predc) / 4) : (int)(offsetof(EncLds, recc) / 4);
        const uint8_t *LB = (const uint8_t *)&S;  // byte offsets into the LDS image (no pointer selects)
        auto ldsw = [&](int dw) -> uint32_t { return ((const uint32_t *)&S)[dw]; };
        const bool carries = type == MI_I16 || (!skip && cbp != 0);
        const uint32_t qflag = (row_carried || carries) ? 0u : 0x80u;  // QPY pending: the row's entry QP
        if (wv == H264MI_ENC_REC_WAVE && lane == 0 && carries && !row_carried && mby + 1 < a.mbh) gran_store(rowq + mby + 1, epoch, (uint32_t)qp);
        row_carried = row_carried || carries;
        if (wv == H264MI_ENC_REC_WAVE && lane < 32) {  // MbInfo (h264mi_types.h), dword `lane`
            // lanes 2..5: the Intra4x4 modes, 7..12: TotalCoeff bytes of blocks 4(l-7)..4(l-7)+3
            const uint32_t ld = ldsw(lane >= 2 && lane < 6 ? O_I4 + lane - 2 : (lane >= 7 && lane < 13 ? O_NZ + lane - 7 : O_I4));
            uint32_t v = (lane == 14 || lane == 31) ? 0u : mvw;
            if (lane == 0) v = (uint32_t)type | (((uint32_t)qp | qflag) << 8) | ((uint32_t)cbp << 16) | ((uint32_t)i16mode << 24);
            if (lane == 1) v = (uint32_t)cmode | (((uint32_t)qpc | qflag) << 8);
            if (lane >= 2 && lane < 6) v = ld;
            if (lane == 6) v = refw;
            if (lane >= 7 && lane < 13) v = skip ? 0u : ld;
            if (lane == 13) v = (uint32_t)(uint16_t)mvdx | ((uint32_t)(uint16_t)mvdy << 16);
            if (lane < 31) info32[(size_t)mbi * 32 + lane] = v;  // (31, the slice word: the row's CAVLC waves, cavlc_row)
            if (lane < 31) gran_store(egr + (size_t)mbi * 128 + 96 + lane, epoch, v);  // -> deblocking row, CAVLC (31: wave 2)
        }
        if (wv == H264MI_ENC_REC_WAVE) stamp(36, t_prev);
        if (wv == 1 && lane < 16 && (idr || !(lane == 8 || lane >= 12))) {  // row-below hand-off (R2 granules; P: 8, 12..15 published at the decision)
            // lanes 0..3 the bottom luma row, 4..7 the bottom chroma rows, 9 the bottom Intra4x4 modes, 10 / 11
            // TotalCoeff of blocks 12..15 / 18, 19, 22, 23 (bytes 2, 3 of dwords 4 and 5)
            const uint32_t ld = ldsw(lane < 4 ? O_REC + 60 + lane
                                              : (lane < 8 ? O_RECC + 16 * ((lane - 4) >> 1) + 14 + (lane & 1)
                                                          : (lane == 9 ? O_I4 + 3 : (lane == 10 ? O_NZ + 3 : O_NZ + 4))));
            const uint32_t ld5 = ldsw(O_NZ + 5);
            uint32_t v = mvw;
            if (lane < 8 || lane == 9) v = ld;
            if (lane == 8) v = (uint32_t)type | ((uint32_t)qp << 8) | (refw & 0xffff0000u);
            if (lane == 10) v = skip ? 0u : ld;
            if (lane == 11) v = skip ? 0u : ((ld >> 16) | (ld5 & 0xffff0000u));
            gran_store(grow + (size_t)mbx * 16 + lane, epoch, v);
        }
        if (wv == 1) stamp(37, t_prev);
        if (wv == 2) {  // coefficient blocks, write-through (sc1): the CAVLC waves of this row read them
            // after granule 127, which follows them (s_waitcnt vmcnt(0) in between). Two lanes per coded
            // block, 16 bytes each: a block leaves as one 32-byte contiguous write (it left as four 8-byte
            // stores at a 32-byte lane stride, four partial-line writes per block). Granule 127 of an MB
            // goes out one MB later, before the next MB's blocks: the wait for the stores' completion
            // then costs nothing (waiting right away held the whole workgroup at the next barrier)
            if (pend127 >= 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane == 0) gran_store(egr + (size_t)pend127 * 128 + 127, epoch, 0u);  // MbInfo dword 31 (pad)
            }
            stamp(38, t_prev);
            const int blk = lane >> 1, half = lane & 1;
            const int16_t *src = nullptr;
            int dst8 = 0;
            if (!skip && lane < 52) {
                if (blk < 16 && S.nnz[blk]) { src = S.lvl[blk]; dst8 = 4 * blk; }
                else if (blk >= 16 && blk < 24 && S.nnz[blk] && (cbp >> 4) == 2) { src = S.lvl[blk]; dst8 = 64 + 4 * (blk - 16); }
                else if (blk == 24 && type == MI_I16) { src = S.ldc; dst8 = 96; }
                else if (blk == 25 && (cbp >> 4) && half == 0) { src = &S.cdc[0][0]; dst8 = 100; }  // 16 bytes: one lane
            }
            if (src) {
                const u32x4 v = *(const u32x4 *)(src + 8 * half);
                const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(uint64_t)(coefg + mbi), (short)0, 0x7fffffff, 0x00020000);
                __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (dst8 + 2 * half) * 8, 0, 16);  // sc1 (write-through)
            }
            pend127 = mbi;
        }
        if (wv == 3 && lane < 48) {  // unfiltered reconstruction -> deblocking row: granule pairs (2k, 2k+1),
            // luma dwords 2 lane, 2 lane + 1 (lanes 0..31), chroma dwords 2m, 2m + 1 (m = lane - 32: plane m >> 3)
            const uint32_t *pw = (const uint32_t *)LB + (lane < 32 ? O_REC + 2 * lane : O_RECC + 16 * ((lane - 32) >> 3) + ((lane - 32) & 7) * 2);
            gran_store2(egr + (size_t)mbi * 128, lane < 32 ? 2 * lane : 64 + 2 * (lane - 32), epoch, pw[0], pw[1]);
        }
        if (wv == 3) stamp(39, t_prev);
        // ---- 5. left-neighbour state for the next MB: pixels in LDS, the rest in (uniform) registers
        L_ref = intra ? -1 : 0; L_mvx = mvx; L_mvy = mvy; L_skip = skip; L_sksad = cur_sk;
        if (!idr && wv == 3 && lane == 63) gbl(D.sksad_cur)[mbi] = cur_sk;
        L_i4 = (uint32_t)uni((int)((uint32_t)(uint8_t)S.i4[3] | ((uint32_t)(uint8_t)S.i4[7] << 8) | ((uint32_t)(uint8_t)S.i4[11] << 16) |
                                   ((uint32_t)(uint8_t)S.i4[15] << 24)));
        stamp(16 + wv, t_prev);
        // the next MB's left samples: nothing reads S.left / S.leftc after the MB's coding path (which ended at a
        // barrier), and the next MB reads them after its own barriers -- one barrier closes the MB
#if H264MI_ENC_ONEBAR
        if (tid < 16) S.left[lane] = LB[4 * O_REC + lane * 16 + 15];
        else if (tid < 32) S.leftc[(lane - 16) >> 3][lane & 7] = LB[4 * O_RECC + 64 * ((lane - 16) >> 3) + (lane & 7) * 8 + 7];
        else if (tid >= 32 && tid < 36) S.pj[(mbx + 1) & 1][tid - 32] = 0;  // the next MB's judge accumulators (EncLds::pj)
        lds_barrier();  // every wave has read S.i4 / S.rec / S.nnz of this MB
#else
        lds_barrier();
        if (tid < 16) S.left[lane] = LB[4 * O_REC + lane * 16 + 15];
        else if (tid < 32) S.leftc[(lane - 16) >> 3][lane & 7] = LB[4 * O_RECC + 64 * ((lane - 16) >> 3) + (lane & 7) * 8 + 7];
        else if (tid >= 32 && tid < 36) S.pj[(mbx + 1) & 1][tid - 32] = 0;
        lds_barrier();
#endif
        lap(10);
    }
    if (wv == 2 && pend127 >= 0) {  // the row's last MB
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) gran_store(egr + (size_t)pend127 * 128 + 127, epoch, 0u);
    }
    // a row without an mb_qp_delta carrier hands on the QP it entered with
    if (!row_carried && mby + 1 < a.mbh && wv == 0) {
        int eq;
        if (row_entry_qp(rowq, mby, !above, slice_qp, epoch, abort_word, &eq) && lane == 0) gran_store(rowq + mby + 1, epoch, (uint32_t)eq);
    }
    if (prof && tid < 40) atomicAdd((unsigned long long *)&a.prof[tid < 16 ? tid : tid + 16], (unsigned long long)s_prof[tid]);
    tl_end();
#undef tid
#undef lane
#undef above
#if H264MI_ENC_XF_LDS
#undef XF
#endif
}

}  // namespace h264mi
