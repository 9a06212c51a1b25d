// enc_bits.inc -- entropy coding and slice/NAL assembly (gfx950).
//
// Replaces OpenH264's CAVLC writer + NAL encapsulation + rate-control frame update inside
// ISVCEncoder::EncodeFrame (openh264_wrapper.cpp:384) and the buffer concatenation of
// copy_encoded_data (:282-311): the output of one frame is one contiguous Annex-B buffer.
//   enc_begin_kernel  : per-stream frame parameters (IDR decision, QP, frame_num/POC, epoch)
//   cavlc_row         : (inside enc_mb_kernel) one wave per macroblock -> macroblock_layer() bits
//                       (9.2 CAVLC), lane per residual block, wave prefix-sum to concatenate
//   enc_pack_kernel   : one workgroup per stream -> mb_skip_run insertion, bit-offset scan,
//                       slice header, RBSP concatenation, emulation prevention (7.4.1), SPS/PPS
//                       for IDR, rate-control update (DESIGN.md §3.6)
namespace h264mi {

// codeNum -> cbp (Table 9-4); the encoder uses the inverse built at compile time
constexpr uint8_t CBP_INTRA_FROM_CODE[48] = {47, 31, 15, 0,  23, 27, 29, 30, 7,  11, 13, 14, 39, 43, 45, 46,
                                             16, 3,  5,  10, 12, 19, 21, 26, 28, 35, 37, 42, 44, 1,  2,  4,
                                             8,  17, 18, 20, 24, 6,  9,  22, 25, 32, 33, 34, 36, 40, 38, 41};
constexpr uint8_t CBP_INTER_FROM_CODE[48] = {0,  16, 1,  2,  4,  8,  32, 3,  5,  10, 12, 15, 47, 7,  11, 13,
                                             14, 6,  9,  31, 35, 37, 42, 44, 33, 34, 36, 40, 39, 43, 45, 46,
                                             17, 18, 20, 24, 19, 21, 26, 28, 23, 27, 29, 30, 22, 25, 38, 41};
struct CbpInv { uint8_t intra[48], inter[48]; };
constexpr CbpInv build_cbp_inv() {
    CbpInv r{};
    for (int i = 0; i < 48; i++) { r.intra[CBP_INTRA_FROM_CODE[i]] = (uint8_t)i; r.inter[CBP_INTER_FROM_CODE[i]] = (uint8_t)i; }
    return r;
}
__constant__ const CbpInv c_CBPINV = build_cbp_inv();
__constant__ const uint8_t c_CBP_INTRA_FROM_CODE[48] = {47, 31, 15, 0,  23, 27, 29, 30, 7,  11, 13, 14, 39, 43, 45, 46,
                                                         16, 3,  5,  10, 12, 19, 21, 26, 28, 35, 37, 42, 44, 1,  2,  4,
                                                         8,  17, 18, 20, 24, 6,  9,  22, 25, 32, 33, 34, 36, 40, 38, 41};
__constant__ const uint8_t c_CBP_INTER_FROM_CODE[48] = {0,  16, 1,  2,  4,  8,  32, 3,  5,  10, 12, 15, 47, 7,  11, 13,
                                                         14, 6,  9,  31, 35, 37, 42, 44, 33, 34, 36, 40, 39, 43, 45, 46,
                                                         17, 18, 20, 24, 19, 21, 26, 28, 23, 27, 29, 30, 22, 25, 38, 41};

// ---------------------------------------------------------------- per-lane MSB-first bit writer into LDS
struct LBits {
    uint32_t *buf;  // this lane's dwords
    uint64_t acc;
    int nacc, nd, total;
};
DEV void lb_init(LBits &b, uint32_t *buf) { b.buf = buf; b.acc = 0; b.nacc = 0; b.nd = 0; b.total = 0; }
DEV void lb_put(LBits &b, uint32_t v, int n) {  // n <= 32
    if (n <= 0) return;
    if (n < 32) v &= (1u << n) - 1u;
    b.acc = (b.acc << n) | v;
    b.nacc += n;
    b.total += n;
    if (b.nacc >= 32) { b.nacc -= 32; b.buf[b.nd++] = (uint32_t)(b.acc >> b.nacc); }
}
DEV void lb_ue(LBits &b, uint32_t v) {
    uint32_t k = v + 1;
    int l = 31 - __clz(k);
    lb_put(b, 0, l);
    lb_put(b, k, l + 1);
}
DEV void lb_se(LBits &b, int v) { lb_ue(b, v > 0 ? (uint32_t)(2 * v - 1) : (uint32_t)(-2 * v)); }
DEV void lb_flush(LBits &b) { if (b.nacc > 0) b.buf[b.nd++] = (uint32_t)(b.acc << (32 - b.nacc)); }

DEV int nc_class(int nc) { return nc < 2 ? 0 : (nc < 4 ? 1 : (nc < 8 ? 2 : 3)); }

// VLC tables of 9.2 staged in LDS per workgroup as (length << 8) | code: a lane's lookups have
// divergent indices, which from __constant__ memory are vector loads on the dependency chain. The
// packed image is built at compile time and copied with 16-byte loads.
struct alignas(16) CavlcTabs {
    uint16_t ct[4][68], ctdc[20], tz[15][16], tzdc[3][4], rb[7][15], pad[7];
};
static_assert(sizeof(CavlcTabs) % 16 == 0, "CavlcTabs copy granule");
// coeff_token (Table 9-5; nC classes 0-2, 2-4, 4-8, >= 8 -- the last is the 6-bit FLC), its chroma
// DC variant, total_zeros (Tables 9-7..9-9) and run_before (Table 9-10)
constexpr CavlcTabs build_cavlc_tabs() {
    constexpr uint8_t CT_LEN[4][68] = {
        {1, 0, 0, 0, 6, 2, 0, 0, 8, 6, 3, 0, 9, 8, 7, 5, 10, 9, 8, 6, 11, 10, 9, 7, 13, 11, 10, 8,
         13, 13, 11, 9, 13, 13, 13, 10, 14, 14, 13, 11, 14, 14, 14, 13, 15, 15, 14, 14, 15, 15, 15, 14,
         16, 15, 15, 15, 16, 16, 16, 15, 16, 16, 16, 16, 16, 16, 16, 16},
        {2, 0, 0, 0, 6, 2, 0, 0, 6, 5, 3, 0, 7, 6, 6, 4, 8, 6, 6, 4, 8, 7, 7, 5, 9, 8, 8, 6,
         11, 9, 9, 6, 11, 11, 11, 7, 12, 11, 11, 9, 12, 12, 12, 11, 12, 12, 12, 11, 13, 13, 13, 12,
         13, 13, 13, 13, 13, 14, 13, 13, 14, 14, 14, 13, 14, 14, 14, 14},
        {4, 0, 0, 0, 6, 4, 0, 0, 6, 5, 4, 0, 6, 5, 5, 4, 7, 5, 5, 4, 7, 5, 5, 4, 7, 6, 6, 4,
         7, 6, 6, 4, 8, 7, 7, 5, 8, 8, 7, 6, 9, 8, 8, 7, 9, 9, 8, 8, 9, 9, 9, 8,
         10, 9, 9, 9, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10},
        {6, 0, 0, 0, 6, 6, 0, 0, 6, 6, 6, 0, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6,
         6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6,
         6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6}};
    constexpr uint8_t CT_CODE[4][68] = {
        {1, 0, 0, 0, 5, 1, 0, 0, 7, 4, 1, 0, 7, 6, 5, 3, 7, 6, 5, 3, 7, 6, 5, 4, 15, 6, 5, 4,
         11, 14, 5, 4, 8, 10, 13, 4, 15, 14, 9, 4, 11, 10, 13, 12, 15, 14, 9, 12, 11, 10, 13, 8,
         15, 1, 9, 12, 11, 14, 13, 8, 7, 10, 9, 12, 4, 6, 5, 8},
        {3, 0, 0, 0, 11, 2, 0, 0, 7, 7, 3, 0, 7, 10, 9, 5, 7, 6, 5, 4, 4, 6, 5, 6, 7, 6, 5, 8,
         15, 6, 5, 4, 11, 14, 13, 4, 15, 10, 9, 4, 11, 14, 13, 12, 8, 10, 9, 8, 15, 14, 13, 12,
         11, 10, 9, 12, 7, 11, 6, 8, 9, 8, 10, 1, 7, 6, 5, 4},
        {15, 0, 0, 0, 15, 14, 0, 0, 11, 15, 13, 0, 8, 12, 14, 12, 15, 10, 11, 11, 11, 8, 9, 10,
         9, 14, 13, 9, 8, 10, 9, 8, 15, 14, 13, 13, 11, 14, 10, 12, 15, 10, 13, 12, 11, 14, 9, 12,
         8, 10, 13, 8, 13, 7, 9, 12, 9, 12, 11, 10, 5, 8, 7, 6, 1, 4, 3, 2},
        {3, 0, 0, 0, 0, 1, 0, 0, 4, 5, 6, 0, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19,
         20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39,
         40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59,
         60, 61, 62, 63}};
    constexpr uint8_t CTDC_LEN[20] = {2, 0, 0, 0, 6, 1, 0, 0, 6, 6, 3, 0, 6, 7, 7, 6, 6, 8, 8, 7};
    constexpr uint8_t CTDC_CODE[20] = {1, 0, 0, 0, 7, 1, 0, 0, 4, 6, 1, 0, 3, 3, 2, 5, 2, 3, 2, 0};
    constexpr uint8_t TZ_LEN[15][16] = {
        {1, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 9}, {3, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 6, 6, 6, 6},
        {4, 3, 3, 3, 4, 4, 3, 3, 4, 5, 5, 6, 5, 6}, {5, 3, 4, 4, 3, 3, 3, 4, 3, 4, 5, 5, 5},
        {4, 4, 4, 3, 3, 3, 3, 3, 4, 5, 4, 5}, {6, 5, 3, 3, 3, 3, 3, 3, 4, 3, 6}, {6, 5, 3, 3, 3, 2, 3, 4, 3, 6},
        {6, 4, 5, 3, 2, 2, 3, 3, 6}, {6, 6, 4, 2, 2, 3, 2, 5}, {5, 5, 3, 2, 2, 2, 4}, {4, 4, 3, 3, 1, 3},
        {4, 4, 2, 1, 3}, {3, 3, 1, 2}, {2, 2, 1}, {1, 1}};
    constexpr uint8_t TZ_CODE[15][16] = {
        {1, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 1}, {7, 6, 5, 4, 3, 5, 4, 3, 2, 3, 2, 3, 2, 1, 0},
        {5, 7, 6, 5, 4, 3, 4, 3, 2, 3, 2, 1, 1, 0}, {3, 7, 5, 4, 6, 5, 4, 3, 3, 2, 2, 1, 0},
        {5, 4, 3, 7, 6, 5, 4, 3, 2, 1, 1, 0}, {1, 1, 7, 6, 5, 4, 3, 2, 1, 1, 0}, {1, 1, 5, 4, 3, 3, 2, 1, 1, 0},
        {1, 1, 1, 3, 3, 2, 2, 1, 0}, {1, 0, 1, 3, 2, 1, 1, 1}, {1, 0, 1, 3, 2, 1, 1}, {0, 1, 1, 2, 1, 3},
        {0, 1, 1, 1, 1}, {0, 1, 1, 1}, {0, 1, 1}, {0, 1}};
    constexpr uint8_t TZDC_LEN[3][4] = {{1, 2, 3, 3}, {1, 2, 2, 0}, {1, 1, 0, 0}};
    constexpr uint8_t TZDC_CODE[3][4] = {{1, 1, 1, 0}, {1, 1, 0, 0}, {1, 0, 0, 0}};
    constexpr uint8_t RB_LEN[7][15] = {{1, 1}, {1, 2, 2}, {2, 2, 2, 2}, {2, 2, 2, 3, 3}, {2, 2, 3, 3, 3, 3},
                                       {2, 3, 3, 3, 3, 3, 3}, {3, 3, 3, 3, 3, 3, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
    constexpr uint8_t RB_CODE[7][15] = {{1, 0}, {1, 1, 0}, {3, 2, 1, 0}, {3, 2, 1, 1, 0}, {3, 2, 3, 2, 1, 0},
                                        {3, 0, 1, 3, 2, 5, 4}, {7, 6, 5, 4, 3, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1}};
    CavlcTabs t{};
    for (int c = 0; c < 4; c++) for (int i = 0; i < 68; i++) t.ct[c][i] = (uint16_t)(CT_LEN[c][i] << 8 | CT_CODE[c][i]);
    for (int i = 0; i < 20; i++) t.ctdc[i] = (uint16_t)(CTDC_LEN[i] << 8 | CTDC_CODE[i]);
    for (int r = 0; r < 15; r++) for (int i = 0; i < 16; i++) t.tz[r][i] = (uint16_t)(TZ_LEN[r][i] << 8 | TZ_CODE[r][i]);
    for (int r = 0; r < 3; r++) for (int i = 0; i < 4; i++) t.tzdc[r][i] = (uint16_t)(TZDC_LEN[r][i] << 8 | TZDC_CODE[r][i]);
    for (int r = 0; r < 7; r++) for (int i = 0; i < 15; i++) t.rb[r][i] = (uint16_t)(RB_LEN[r][i] << 8 | RB_CODE[r][i]);
    return t;
}
__constant__ const CavlcTabs c_CAVLC_TABS = build_cavlc_tabs();
DEV void cavlc_tabs_load(CavlcTabs &T) {
    const u32x4 *src = (const u32x4 *)&c_CAVLC_TABS;
    u32x4 *dst = (u32x4 *)&T;
    for (int i = threadIdx.x; i < (int)(sizeof(CavlcTabs) / 16); i += blockDim.x) dst[i] = src[i];
}
DEV void lb_vlc(LBits &b, uint16_t e) { lb_put(b, e & 255u, e >> 8); }

// 9.2 residual_block_cavlc() of the scan-ordered coefficients coef[0..maxnum) (this lane's LDS
// row); loops run over the nonzero coefficients only (most blocks hold a few).
DEV void cavlc_block(LBits &b, const CavlcTabs &T, const int16_t *coef, int maxnum, int nc) {
    int last = -1, tc = 0, t1 = 0;
    for (int i = maxnum - 1; i >= 0; i--) if (coef[i]) { last = i; break; }
    for (int i = 0; i <= last; i++) tc += coef[i] != 0;
    // trailing ones: from the highest frequency down, up to 3 consecutive |level| == 1
    for (int i = last, seen = 0; i >= 0 && seen < 3; i--) {
        if (!coef[i]) continue;
        if (iabs(coef[i]) == 1) { t1++; seen++; } else break;
    }
    const int tz = last >= 0 ? last + 1 - tc : 0;
    lb_vlc(b, nc == -1 ? T.ctdc[tc * 4 + t1] : T.ct[nc_class(nc)][tc * 4 + t1]);
    if (!tc) return;
    int sl = (tc > 10 && t1 < 3) ? 1 : 0;
    int idx = 0;  // index among nonzero coefficients, highest frequency first
    for (int i = last; i >= 0; i--) {
        const int l = coef[i];
        if (!l) continue;
        if (idx < t1) { lb_put(b, l < 0, 1); idx++; continue; }
        int code = l > 0 ? 2 * l - 2 : -2 * l - 1;
        if (idx == t1 && t1 < 3) code -= 2;
        if (sl == 0) {
            if (code < 14) lb_put(b, 1, code + 1);
            else if (code < 30) { lb_put(b, 1, 15); lb_put(b, code - 14, 4); }
            else { lb_put(b, 1, 16); lb_put(b, code - 30, 12); }
        } else {
            if (code < (15 << sl)) { lb_put(b, 1, (code >> sl) + 1); lb_put(b, code & ((1 << sl) - 1), sl); }
            else { lb_put(b, 1, 16); lb_put(b, code - (15 << sl), 12); }
        }
        if (sl == 0) sl = 1;
        if (iabs(l) > (3 << (sl - 1)) && sl < 6) sl++;
        idx++;
    }
    if (tc < maxnum) lb_vlc(b, nc == -1 ? T.tzdc[tc - 1][tz] : T.tz[tc - 1][tz]);
    // run_before, from the highest-frequency coefficient down
    int zl = tz, k = 0;
    for (int i = last; i >= 0 && zl > 0 && k < tc - 1; i--) {
        if (!coef[i]) continue;
        int r = 0, j = i - 1;
        while (j >= 0 && coef[j] == 0) { r++; j--; }
        lb_vlc(b, T.rb[zl > 7 ? 6 : zl - 1][r]);
        zl -= r;
        k++;
    }
}

// ---------------------------------------------------------------- CAVLC of one macroblock (one wave)
// Runs inside enc_mb_kernel: waves 1 and 2 of each deblocking workgroup code the macroblocks of its
// row (alternately) as the MB-row encoder publishes them. Lanes: 0 header | 1 luma DC (I16) |
// 2..17 luma blocks (blkIdx order) | 18,19 chroma DC | 20..27 chroma AC; prefix sum of the lane
// lengths, LDS merge, per-MB bit slot (D.mbbits / D.mblen, read by enc_pack_kernel).
struct CavlcWaveLds {
    uint32_t bits[28][24];
    uint32_t out[H264MI_MB_SLOT_DWORDS];
    alignas(16) int16_t coef[28][16];
    alignas(16) MbInfo cur, left, top;
};
// MbCoef byte offset of the block lane codes (-1: none): 1 luma DC | 2..17 luma | 18,19 chroma DC
// (both planes, 16 bytes) | 20..27 chroma AC
DEV int cavlc_lane_off(int lane) {
    if (lane == 1) return 768;
    if (lane >= 2 && lane < 18) return 32 * BLK2RAS[lane - 2];
    if (lane == 18 || lane == 19) return 800;
    if (lane >= 20 && lane < 28) return 512 + 32 * (lane - 20);
    return -1;
}
// ic / il / it: MbInfo dword `lane` (lanes 0..31) of the MB, its left and its top neighbour;
// c[0..3]: the 32 bytes at the lane's block offset (whatever is stored there; used only if coded)
// dqp: this MB's mb_qp_delta (written when it carries one); above: the MB above is in this MB's slice
DEV void cavlc_code_mb(const CavlcTabs &T, CavlcWaveLds &W, CONSTANT const EncDesc &D, int mbi, int mbx, bool above, int idr,
                       uint32_t ic, uint32_t il, uint32_t it, const uint64_t *c, int dqp, uint32_t bitg_epoch) {
    const int lane = threadIdx.x & 63;
    MbInfo &Cm = W.cur, &Lm = W.left, &Tm = W.top;
    if (lane < 32) {
        ((uint32_t *)&Cm)[lane] = ic;
        ((uint32_t *)&Lm)[lane] = il;
        ((uint32_t *)&Tm)[lane] = it;
    }
    wave_lds_sync();
    const int type = uni(Cm.type);
    if (type == MI_PSKIP) {
        if (lane == 0) { gbl(D.mblen)[mbi] = 0; if (bitg_epoch) gran_store(gbl(D.bitg) + mbi, bitg_epoch, 0u); }
        return;
    }
    const int cbp = uni(Cm.cbp), cbpl = cbp & 15, cbpc = cbp >> 4;
    const bool i16 = type == MI_I16;
    // this lane's block: coded flag, stored (TotalCoeff > 0; MbCoef holds only those), maxnum, AC shift, nC
    int maxnum = 0, nc = 0, sh = 0;
    bool coded = false, stored = false;
    if (lane == 1) { coded = i16; maxnum = 16; stored = true; }
    else if (lane >= 2 && lane < 18) {
        const int blk = lane - 2, ras = BLK2RAS[blk];
        coded = i16 ? cbpl != 0 : ((cbpl >> (blk >> 2)) & 1) != 0;
        maxnum = i16 ? 15 : 16; sh = i16 ? 1 : 0;
        stored = Cm.nnz[ras] != 0;
    } else if (lane >= 18 && lane < 20) { coded = cbpc != 0; maxnum = 4; nc = -1; stored = true; }
    else if (lane >= 20 && lane < 28) {
        const int pl = (lane - 20) >> 2, bb = (lane - 20) & 3;
        coded = cbpc == 2; maxnum = 15; sh = 1;
        stored = Cm.nnz[16 + 4 * pl + bb] != 0;
    }
    uint32_t cw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (coded && stored) {
#pragma unroll
        for (int k = 0; k < 4; k++) { cw[2 * k] = (uint32_t)c[k]; cw[2 * k + 1] = (uint32_t)(c[k] >> 32); }
        if (lane == 19) { cw[0] = cw[2]; cw[1] = cw[3]; }
        if (lane == 18 || lane == 19) { cw[2] = cw[3] = cw[4] = cw[5] = cw[6] = cw[7] = 0; }
        if (sh) {  // AC blocks: coefficient k is stored at scan index k + 1
#pragma unroll
            for (int i = 0; i < 7; i++) cw[i] = __builtin_amdgcn_alignbit(cw[i + 1], cw[i], 16);
            cw[7] >>= 16;
        }
    }
    if (lane < 28) {
        u32x4 *row = (u32x4 *)W.coef[lane];
        row[0] = u32x4{cw[0], cw[1], cw[2], cw[3]};
        row[1] = u32x4{cw[4], cw[5], cw[6], cw[7]};
    }
    if (lane >= 1 && lane < 18) {  // luma nC (9.2.1): blkA / blkB TotalCoeff
        const int ras = lane == 1 ? 0 : BLK2RAS[lane - 2], bx = ras & 3, by = ras >> 2;
        int na = -1, nb = -1;
        if (bx > 0) na = Cm.nnz[ras - 1]; else if (mbx > 0) na = Lm.nnz[ras + 3];
        if (by > 0) nb = Cm.nnz[ras - 4]; else if (above) nb = Tm.nnz[ras + 12];
        nc = (na >= 0 && nb >= 0) ? (na + nb + 1) >> 1 : (na >= 0 ? na : (nb >= 0 ? nb : 0));
    } else if (lane >= 20 && lane < 28) {
        const int pl = (lane - 20) >> 2, bb = (lane - 20) & 3, base = 16 + 4 * pl, bx = bb & 1, by = bb >> 1;
        int na = -1, nb = -1;
        if (bx > 0) na = Cm.nnz[base + bb - 1]; else if (mbx > 0) na = Lm.nnz[base + bb + 1];
        if (by > 0) nb = Cm.nnz[base + bb - 2]; else if (above) nb = Tm.nnz[base + bb + 2];
        nc = (na >= 0 && nb >= 0) ? (na + nb + 1) >> 1 : (na >= 0 ? na : (nb >= 0 ? nb : 0));
    }
    int len = 0;
    if (lane < 28) {
        LBits b;
        lb_init(b, W.bits[lane]);
        if (lane == 0) {
            // macroblock_layer() header (7.3.5)
            const int moff = idr ? 0 : 5;
            if (type == MI_I4) {
                lb_ue(b, moff);
                for (int blk = 0; blk < 16; blk++) {
                    const int ras = BLK2RAS[blk], bx = ras & 3, by = ras >> 2;
                    const int ma = bx > 0 ? Cm.i4mode[ras - 1] : (mbx > 0 ? Lm.i4mode[ras + 3] : -1);
                    const int mb = by > 0 ? Cm.i4mode[ras - 4] : (above ? Tm.i4mode[ras + 12] : -1);
                    const int pm = (ma < 0 || mb < 0) ? 2 : min(ma, mb);
                    const int m = Cm.i4mode[ras];
                    if (m == pm) lb_put(b, 1, 1);
                    else { lb_put(b, 0, 1); lb_put(b, m < pm ? m : m - 1, 3); }
                }
                lb_ue(b, Cm.cmode);
                lb_ue(b, c_CBPINV.intra[cbp]);
                if (cbp) lb_se(b, dqp);
            } else if (i16) {
                lb_ue(b, moff + 1 + Cm.i16mode + 4 * cbpc + 12 * (cbpl ? 1 : 0));
                lb_ue(b, Cm.cmode);
                lb_se(b, dqp);
            } else {
                lb_ue(b, 0);
                lb_se(b, Cm.mvd[0]);
                lb_se(b, Cm.mvd[1]);
                lb_ue(b, c_CBPINV.inter[cbp]);
                if (cbp) lb_se(b, dqp);
            }
        } else if (coded) {
            cavlc_block(b, T, W.coef[lane], maxnum, nc);
        }
        lb_flush(b);
        len = b.total;
    }
    // exclusive prefix sum of lengths over lanes 0..27
    int incl = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    const int boff = incl - len;
    const int total = __shfl(incl, 63);
    const int nd = (total + 31) >> 5;
    uint32_t *out = W.out;
    for (int i = lane; i < nd; i += 64) out[i] = 0;
    wave_lds_sync();
    if (lane < 28 && len > 0) {
        const int w0 = boff >> 5, bsh = boff & 31, n = (len + 31) >> 5;
        for (int k = 0; k < n; k++) {
            uint32_t v = W.bits[lane][k];
            if (k == n - 1 && (len & 31)) v &= ~0u << (32 - (len & 31));
            atomicOr(&out[w0 + k], v >> bsh);
            if (bsh) atomicOr(&out[w0 + k + 1], v << (32 - bsh));
        }
    }
    wave_lds_sync();
    GLOBAL uint32_t *dst = gbl(D.mbbits) + (size_t)mbi * H264MI_MB_SLOT_DWORDS;
    for (int i = lane; i < nd; i += 64) dst[i] = out[i];
    if (lane == 0) {
        gbl(D.mblen)[mbi] = (uint32_t)total;
        if (bitg_epoch) gran_store(gbl(D.bitg) + mbi, bitg_epoch, (uint32_t)total);  // -> the next GOM's QP (gom_row_qp)
    }
}


// The CAVLC of MB row mby, macroblocks x0, x0 + dx, ...: each waits for the MB record granules the
// MB-row encoder publishes (96..127 of its 128; granule 127 follows its coefficient stores, which are
// write-through (sc1), so sc1 loads of them after the granule see them -- MI355X_MICROARCH.md
// inter-workgroup visibility, valid forms); the neighbours' records are granules too.
DEV void cavlc_row(CavlcTabs &T, CavlcWaveLds &W, CONSTANT const EncDesc &D, int mbw, int mbh, int mby, int x0, int dx,
                   uint32_t epoch, int32_t *abort_word, bool bitg) {
    const int lane = threadIdx.x & 63;
    // a slice's first row (DESIGN.md §3.7): no nC / Intra4x4 mode context from the row above, which is not waited
    // for, and the slice QP as the row's entry QP
    const int nsl = uni(D.st->cur_slices), sl_row0 = slice_first_row(mbh, nsl, slice_of_row(mbh, nsl, mby));
    const bool above = mby > sl_row0;
    // the slice word of the row's MB records (MbInfo dword 31, MB_SLICE_FIRST: the slice's first MB; the loop-filter
    // bits stay 0) is written here, off the MB rows' critical path
    GLOBAL uint32_t *info32 = gbl((uint32_t *)D.info);
    {   // this wave's copy of the VLC tables (the other CAVLC wave writes identical values)
        const u32x4 *src = (const u32x4 *)&c_CAVLC_TABS;
        u32x4 *dst = (u32x4 *)&T;
        for (int i = lane; i < (int)(sizeof(CavlcTabs) / 16); i += 64) dst[i] = src[i];
    }
    GLOBAL const uint64_t *egr = gbl((const uint64_t *)D.egran);
    GLOBAL const uint8_t *coefb = gbl((const uint8_t *)D.coef);
    const int idr = uni(D.st->cur_idr);
    const int off = cavlc_lane_off(lane);
    for (int mbx = x0; mbx < mbw; mbx += dx) {
        const int mbi = mby * mbw + mbx;
        uint32_t ic = 0, il = 0, it = 0;
        if (!gran_wait(egr + (size_t)mbi * 128 + 96, 32, epoch, &ic, abort_word)) return;
        if (lane == 0) info32[(size_t)mbi * 32 + 31] = (uint32_t)(sl_row0 * mbw);
        if (mbx > 0 && !gran_wait(egr + (size_t)(mbi - 1) * 128 + 96, 32, epoch, &il, abort_word)) return;
        if (above && !gran_wait(egr + (size_t)(mbi - mbw) * 128 + 96, 32, epoch, &it, abort_word)) return;
        uint64_t c[4] = {0, 0, 0, 0};
        if (off >= 0) {
            const uint64_t *cp = (const uint64_t *)(coefb + (size_t)mbi * sizeof(MbCoef) + off);
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] = __hip_atomic_load(cp + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // mb_qp_delta (7.4.5, DESIGN.md §3.6): a carrier's QP (never flagged) relative to the QPY of
        // the MB before it in raster order -- the left record's, or the row's entry QP at the row
        // start or when the left record is flagged 0x80 (no carrier before it in the row)
        const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)ic, 0), l0 = (uint32_t)__builtin_amdgcn_readlane((int)il, 0);
        const int ty = (int)(c0 & 255), cbp = (int)((c0 >> 16) & 255);
        int dqp = 0;
        if (ty == MI_I16 || (ty != MI_PSKIP && cbp != 0)) {
            int pred = (int)((l0 >> 8) & 0x7f);
            if ((mbx == 0 || ((l0 >> 8) & 0x80u)) && !row_entry_qp(gbl((const uint64_t *)D.rowq), mby, !above, uni(D.st->cur_qp), epoch, abort_word, &pred))
                return;
            dqp = (((int)((c0 >> 8) & 0x7f) - pred + 26 + 52) % 52) - 26;
        }
        cavlc_code_mb(T, W, D, mbi, mbx, above, idr, ic, il, it, c, dqp, bitg ? epoch : 0u);
    }
}

// ---------------------------------------------------------------- per-stream frame begin: frame complexity,
// skip decision and the rate control's picture init (DESIGN.md §3.6; oracle rc_judge_skip / rc_complexity /
// rc_picture_init, restated from h264.wasm funcs 589, 1258, 1254, 910, 1226)
struct BeginLaunch {
    int S, w, h, cw, ch, K;      // K workgroups per stream share its GOMs
    const EncDesc *desc;
    uint32_t *ticket;            // enc_mb_kernel's ticket counters (zeroed here)
    const uint8_t *src_base;     // the frames of this step (tight I420), stream s at src_base + s * src_stride
    size_t src_stride;
    int src_vec;                 // 16-byte source loads (w % 16 == 0, aligned frames)
    uint32_t *done;              // per stream: workgroups finished (the last one runs the picture init, then zeroes it)
    int slices;                  // slices per picture of this frame (h264mi_enc_set_slices), latched into EncState::cur_slices
};
DEV int rc_qstep2qp(int32_t qstep) {  // RcConvertQStep2Qp (thresholds c_RC_QP_THR, h264mi_dev.h)
    if (qstep < 64) return 0;
    int q = 0;
    while (q < 52 && qstep >= c_RC_QP_THR[q]) q++;
    return q;
}
DEV int64_t rc_cmplx_ratio(int64_t fc, int64_t mean) {  // WELS_DIV_ROUND64(fc * 100, mean), clipped to 80..120
    int64_t r = mean == 0 ? fc * 100 : (fc * 100 + mean / 2) / mean;
    r = r <= 80 ? 80 : r;
    return r >= 120 ? 120 : r;
}
DEV int32_t rc_qstep_model(int64_t cmplx, int64_t ratio, int target) {  // WELS_DIV_ROUND64(cmplx * ratio, target * 100)
    const int64_t v = target == 0 ? cmplx * ratio : ((int64_t)(target * 50) + cmplx * ratio) / (int64_t)(target * 100);
    return (int32_t)(uint32_t)(uint64_t)v;
}
DEV void rc_init_vgop(RcState &r) {  // RcInitVGop with bFixRCOverShoot
    const int t = r.remaining + (r.gop_index - r.gop_num) * (r.vgop_bits / r.gop_num);
    r.remaining = (t < 0 ? t : 0) + (r.bpf << 3);
    r.vgop_bits = r.remaining;
    r.gop_index = 0;
    r.frame_coded_in_vgop = 0;
    r.remaining_weights = r.gop_num * 2000;  // WEIGHT_MULTIPLY
}
// the begin logic of one stream (one thread), once its frame complexity is known
DEV void enc_begin_stream(EncState *st, uint32_t *gomc, int slices) {
    RcState &r = st->rc;
    // a frame whose kernels reported an error (wavefront timeout, overflow) produced no output, so
    // the decoder never saw the picture the encoder now holds as its reference: restart with an IDR
    const int idr = st->first || st->force_idr || st->err != 0;
    st->epoch = st->epoch + 1;
    st->err = 0;
    // the frame's slice count (the host's value when the frame step was issued, validated by h264mi_enc_set_slices):
    // latched here, so that every kernel of the frame reads one value whatever the setter does meanwhile
    st->cur_slices = slices < 1 ? 1 : slices;
    // frame skip (func 589's check + CheckFrameSkipBasedMaxbr, func 1258): the update's flag, else the buffer
    // above its size with the run of skipped frames at most (round(fullness / bits per frame) + 1) >> 1
    int skip = 0;
    if (r.skip_flag) skip = 1;
    else if (r.skip_en) {
        const int64_t q = r.bpf == 0 ? r.fullness : (r.fullness + r.bpf / 2) / r.bpf;
        const int pred = ((int32_t)(uint32_t)(uint64_t)q + 1) >> 1;
        skip = pred >= r.continual_skip && r.fullness > r.buffer_size_skip;
    }
    if (skip) { r.skip_flag = 0; r.continual_skip++; }
    if (skip && !idr) {  // WelsRcPostFrameSkipping (func 1254); the reference and the source picture stay
        st->cur_skip = 1;
        r.fullness -= r.bpf;
        r.remaining += r.bpf;
        if (r.fullness < 0) r.fullness = 0;
        st->skipped = st->skipped + 1;
        return;
    }
    st->cur_skip = 0;
    st->first = 0; st->force_idr = 0;
    if (idr) { st->frame_num = 0; st->poc = 0; st->idr_pic_id = (st->idr_pic_id + 1) & 0xffff; }
    st->cur_idr = idr;
    // the frame's complexity: GOM SADs (P) or GOM variances (I), uint32 sums (func 910)
    uint32_t fc = 0;
    for (int g = 0; g < r.gom_count; g++)
        fc += __hip_atomic_load(gomc + (idr ? r.gom_count : 0) + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    r.frame_cmplx = (int64_t)fc;
    r.prev_idx ^= 1;  // this frame's source becomes the preprocessing's reference picture
    // WelsRcPictureInitGom (func 1226)
    r.continual_skip = 0;
    if (idr && r.idr_num == 0) {  // RcInitRefreshParameter (+ RcInitTlWeight, RcUpdateBitrateFps)
        r.intra_cmplx = 0; r.intra_mb_count = 0; r.intra_cmplx_mean = 0;
        r.pframe_num = 0; r.linear_cmplx = 0; r.frame_cmplx_mean = 0;
        r.fullness = 0; r.gop_index = 0; r.vgop_bits = 0; r.remaining = 0;
        r.bpf = r.c_bpf; r.min_bits_tl = r.c_min_bits_tl; r.max_bits_tl = r.c_max_bits_tl; r.buffer_size_skip = r.c_buffer_size_skip;
        rc_init_vgop(r);
    }
    if (r.gop_index == r.gop_num || idr) rc_init_vgop(r);  // RcUpdateTemporalZero
    r.gop_index++;
    r.bits_level = 0;  // RcDecideTargetBits
    if (idr) r.target = r.idr_num ? 400 * r.bpf / 100 : r.bpf << 2;
    else {
        const int rw = r.remaining_weights, wt = r.tl_weight;
        int tb;
        if (rw >= wt) tb = rw == 0 ? (int)(uint32_t)((uint64_t)(uint32_t)r.remaining * (uint64_t)(uint32_t)wt)
                                   : (int)(((int64_t)(rw / 2) + (int64_t)r.remaining * wt) / rw);
        else tb = r.remaining;
        if (tb <= 0 && !r.skip_en) r.bits_level = 2;
        r.target = clip3(r.min_bits_tl, r.max_bits_tl, tb);
    }
    r.remaining_weights -= r.tl_weight;
    int q;
    if (idr) {  // RcCalculateIdrQp
        if (r.idr_num == 0) q = r.idr_table_qp;
        else {
            if (r.nmb != r.intra_mb_count) r.intra_cmplx = r.intra_cmplx * r.nmb / r.intra_mb_count;
            q = rc_qstep2qp(rc_qstep_model(r.intra_cmplx, rc_cmplx_ratio(r.frame_cmplx, r.intra_cmplx_mean), r.target));
        }
        q = clip3(r.idr_lo, r.idr_hi, q);
        r.init_qp = q;
        r.max_frame_qp = clip3(r.idr_lo, r.idr_hi, q + 3);
        r.min_frame_qp = clip3(r.idr_lo, r.idr_hi, q - 3);
    } else {    // RcCalculatePictureQp
        if (r.pframe_num == 0) q = r.init_qp;
        else if (r.bits_level == 2) q = r.last_qscale + 3;
        else {
            r.qstep = rc_qstep_model(r.linear_cmplx, rc_cmplx_ratio(r.frame_cmplx, r.frame_cmplx_mean), r.target);
            q = rc_qstep2qp(r.qstep);
        }
        r.min_frame_qp = clip3(12, 42, r.last_qscale - 3);   // iFrameDeltaQpLower / Upper at iRcVaryRatio 10
        r.max_frame_qp = clip3(12, 42, r.last_qscale + 5);
        q = clip3(r.min_frame_qp, r.max_frame_qp, q);
    }
    r.last_qscale = q;
    r.qstep = c_RC_QSTEP[q];
    st->cur_qp = q;
    // RcInitSliceInformation / the slice's RC init: the slice's target bits (the exact GOM rule's budget)
    const int bpm = (int)(uint32_t)(uint64_t)(r.nmb == 0 ? (int64_t)r.target * 100 : ((int64_t)(r.nmb / 2) + (int64_t)r.target * 100) / r.nmb);
    r.target_bits_slice = (int)(uint32_t)(uint64_t)(((int64_t)r.nmb * bpm + 50) / 100);
}
// grid (K, S): workgroup k of stream s takes GOMs k, k + K, ...; per GOM the luma SAD against the last coded
// frame's source and the sum / square sum (their GOM_VAR value), the coded-size source (edge-replicated) copied
// to the other source buffer; the stream's last workgroup (an agent-scope counter) runs enc_begin_stream.
__global__ __launch_bounds__(256) void enc_begin_kernel(BeginLaunch a) {
    const int s = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
    if (a.ticket && s == 0 && k == 0 && tid < 16) a.ticket[tid] = 0;  // enc_mb_kernel's ticket counters (0; 8..15 per XCD)
    const EncDesc &D = a.desc[s];
    EncState *st = D.st;
    const RcState &r = st->rc;
    const int G = r.gom_count, mpg = r.mb_per_gom, mbw = r.mbw, nmb = r.nmb, pi = r.prev_idx;
    const uint8_t *src = a.src_base + (size_t)s * a.src_stride;
    const uint8_t *ref = D.psrc[pi];
    uint8_t *cpy = D.psrc[pi ^ 1];
    __shared__ uint32_t s_red[3][8];
    for (int g = k; g < G; g += a.K) {
        const int m0 = g * mpg, m1 = min((g + 1) * mpg, nmb);
        // the GOM's MBs are whole MB rows (mb_per_gom is a multiple of mbw): luma rows y0..y1, chunks of 16 columns
        const int y0 = (m0 / mbw) * 16, y1 = ((m1 + mbw - 1) / mbw) * 16, cpr = a.cw >> 4;
        uint32_t sad = 0, sum = 0, sq = 0;
        for (int c = tid; c < (y1 - y0) * cpr; c += 256) {
            const int y = y0 + c / cpr, x = (c % cpr) * 16, sy = min(y, a.h - 1);
            u32x4 cv;
            if (a.src_vec && x + 16 <= a.w) cv = *(const u32x4 *)(src + (size_t)sy * a.w + x);
            else {
                uint32_t wd[4];
                for (int j = 0; j < 4; j++) {
                    uint32_t v = 0;
                    for (int b = 0; b < 4; b++) v |= (uint32_t)src[(size_t)sy * a.w + min(x + 4 * j + b, a.w - 1)] << (8 * b);
                    wd[j] = v;
                }
                cv = u32x4{wd[0], wd[1], wd[2], wd[3]};
            }
            const u32x4 rv = *(const u32x4 *)(ref + (size_t)y * a.cw + x);
            *(u32x4 *)(cpy + (size_t)y * a.cw + x) = cv;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t cw4 = cv[j], rw4 = rv[j];
                sad = __builtin_amdgcn_sad_u8(cw4, rw4, sad);
#pragma unroll
                for (int b = 0; b < 4; b++) { const uint32_t p = (cw4 >> (8 * b)) & 255; sum += p; sq += p * p; }
            }
        }
        // workgroup sums (uint32, wrapping like the wasm's)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { sad += __shfl_down(sad, o); sum += __shfl_down(sum, o); sq += __shfl_down(sq, o); }
        if ((tid & 63) == 0) { s_red[0][tid >> 6] = sad; s_red[1][tid >> 6] = sum; s_red[2][tid >> 6] = sq; }
        __syncthreads();
        if (tid == 0) {
            uint32_t a0 = 0, a1 = 0, a2 = 0;
            for (int wv = 0; wv < 4; wv++) { a0 += s_red[0][wv]; a1 += s_red[1][wv]; a2 += s_red[2][wv]; }
            const uint32_t first_row = (uint32_t)(min((m0 / mbw + 1) * mbw, m1) - m0);
            __hip_atomic_store(D.gomc + g, a0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(D.gomc + G + g, a2 - (a1 * a1) / (first_row << 8), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
    }
    if (tid == 0) {
        const uint32_t n = __hip_atomic_fetch_add(a.done + s, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (n + 1 == (uint32_t)a.K) {
            enc_begin_stream(st, D.gomc, a.slices);
            __hip_atomic_store(a.done + s, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---------------------------------------------------------------- slice assembly
struct PackLaunch { int mbw, mbh, S; const EncDesc *desc; };

DEV void bits_or(uint32_t *rb, int pos, uint32_t v, int n) {  // OR n (<=32) bits of v at bit pos
    if (n <= 0) return;
    if (n < 32) v &= (1u << n) - 1u;
    uint64_t x = (uint64_t)v << (64 - n);  // left aligned in 64 bits
    int w = pos >> 5;
    int sh = (int)(pos & 31);
    uint64_t y = x >> sh;
    uint32_t hi = (uint32_t)(y >> 32), lo = (uint32_t)y;
    if (hi) atomicOr(&rb[w], hi);
    if (lo) atomicOr(&rb[w + 1], lo);
    if (sh + n > 64) {
        uint32_t t = (uint32_t)(x << (64 - sh));
        if (t) atomicOr(&rb[w + 2], t);
    }
}
DEV void bits_ue(uint32_t *rb, int pos, uint32_t v) {  // writes ue(v) at pos (the zero prefix is implicit)
    uint32_t k = v + 1;
    int l = 31 - __clz(k);
    bits_or(rb, pos + l, k, l + 1);
}

// Workgroup-wide scans for the 1024-thread pack kernel: a wave scan on shuffles, the 16 wave totals
// scanned by wave 0 through LDS (two barriers per scan instead of a Hillis-Steele loop's twenty).
// 256 threads (one wave per SIMD, <= 64 VGPRs): the kernel must fit beside the decoder's resident
// wavefront waves, or its dispatch waits for a whole free CU
#ifndef H264MI_PACK_THREADS  // diagnostics: 512 / 1024 measured the same at 32 streams (3753-3767 frames/s,
#define H264MI_PACK_THREADS 256  // profiles/round3/ab_pack): the pack is not what the step waits on
#endif
constexpr int PACK_THREADS = H264MI_PACK_THREADS, PACK_WAVES = PACK_THREADS / 64;
static_assert(PACK_THREADS % 64 == 0 && PACK_WAVES <= 64, "block_excl_scan: one wave scans the wave totals");
template <bool MAX> DEV int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o);
        if (lane >= o) v = MAX ? max(v, t) : v + t;
    }
    return v;
}
// exclusive scan (sum, or max with identity -1) over the workgroup; *total = the inclusive total
template <bool MAX> DEV int block_excl_scan(int v, int *s_w, int *total) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int inc = wave_incl_scan<MAX>(v);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    if (wv == 0) {
        int x = lane < PACK_WAVES ? s_w[lane] : (MAX ? -1 : 0);
        x = wave_incl_scan<MAX>(x);
        if (lane < PACK_WAVES) s_w[lane] = x;
    }
    __syncthreads();
    const int before = wv > 0 ? s_w[wv - 1] : (MAX ? -1 : 0);
    *total = s_w[PACK_WAVES - 1];
    __syncthreads();  // s_w is reused by the next scan
    if (MAX) {
        const int up = __shfl_up(inc, 1);  // every lane takes part: a bpermute reading an inactive lane returns 0
        return max(before, lane > 0 ? up : -1);
    }
    return before + inc - v;
}

// ---------------------------------------------------------------- exact GOM rate control (opt-in, EncLaunch::gomr)
// OpenH264's per-GOM QP (WelsRcMbInitGom, h264.wasm func 1215: RcCalculateGomQp + RcGomTargetBits; the bits come
// from WelsRcMbInfoUpdateGom, func 1206; oracle rc_mb_init_gom) for P frames: the QP of GOM k's MB rows depends on
// the bits of every MB before it, so GOM k's first row waits for the bits of every MB of GOM k - 1 (granules the
// CAVLC waves publish, skip runs counted like the slice writer: ue(run) with the MB that follows the run) and for
// GOM k - 1's state (granules gomst[4 (k - 1) ...]: QP, slice bits before it, its target bits, last coded MB + 1),
// then publishes its own. The launch's tickets are GOM-major (the GOM's encoder rows, then its deblocking / CAVLC
// rows), so every wait is on lower tickets. Runs on wave 0 of the row's workgroup; returns the row's QP, or -1 when
// a wait gave up (the frame is aborting).
DEV int gom_row_qp(CONSTANT const EncDesc &D, EncState *st, int mby, int mbw, int R, uint32_t epoch, int32_t *abort_word) {
    const int lane = threadIdx.x & 63;
    const RcState &r = st->rc;
    const int k = mby / R, nmb = r.nmb, mpg = mbw * R, G = (nmb + mpg - 1) / mpg, last_g = (nmb - 1) / mpg;
    GLOBAL uint64_t *gs = gbl(D.gomst);
    if (mby % R != 0) {  // a later row of the GOM: the GOM's QP from its first row
        uint32_t q = 0;
        if (!gran_wait(gs + 4 * k, 1, epoch, &q, abort_word)) return -1;
        return (int)__builtin_amdgcn_readlane((int)q, 0);
    }
    const int tslice = uni(r.target_bits_slice), qmin = uni(r.min_frame_qp), qmax = uni(r.max_frame_qp);
    int qp, fb, last;
    if (k == 0) { qp = uni(st->cur_qp); fb = 0; last = -1; }
    else {
        uint32_t v = 0;
        if (!gran_wait(gs + 4 * (k - 1), 4, epoch, &v, abort_word)) return -1;
        const int qprev = __builtin_amdgcn_readlane((int)v, 0), fbprev = __builtin_amdgcn_readlane((int)v, 1);
        const int gtprev = __builtin_amdgcn_readlane((int)v, 2);
        last = __builtin_amdgcn_readlane((int)v, 3) - 1;
        // the bits of GOM k - 1's MBs, each coded MB with the ue(mb_skip_run) written before it
        const int m0 = (k - 1) * mpg, m1 = min(k * mpg, nmb);
        int gbits = 0;
        for (int base = m0; base < m1; base += 64) {
            uint32_t len = 0;
            if (!gran_wait(gbl(D.bitg) + base, min(64, m1 - base), epoch, &len, abort_word)) return -1;
            const int i = base + lane;
            const bool coded = i < m1 && len > 0;
            const int inc = wave_incl_scan<true>(coded ? i : -1);
            const int up = __shfl_up(inc, 1);  // every lane takes part (a bpermute reading an inactive lane returns 0)
            const int before = max(last, lane > 0 ? up : -1);
            int b = coded ? (int)len + ue_len((uint32_t)(i - before - 1)) : 0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) b += __shfl_xor(b, o);
            gbits += b;
            last = max(last, __builtin_amdgcn_readlane(inc, 63));
        }
        fb = fbprev + gbits;
        // RcCalculateGomQp: +2 / +1 / -1 at bit ratios 0.8409 / 0.9439 / 1.06 (the -2 branch is unreachable)
        int d = 2;
        const int left = tslice - fb;
        if (left > 0) {
            const int64_t tleft = (int64_t)left + gbits - gtprev;
            if (tleft > 0) {
                const uint64_t ratio = (uint64_t)((int64_t)left * 10000) / (uint64_t)(tleft + 1);
                if (ratio >= 8409) d = ratio < 9439 ? 1 : -(int)(ratio > 10600);
            }
        }
        qp = clip3(qmin, qmax, qprev + d);
    }
    // RcGomTargetBits: the bits left, shared over the GOMs still to code by this frame's GOM SADs
    int left = tslice - fb, gt;
    if (left <= 0) gt = 0;
    else if (last_g <= k) gt = left;
    else {
        int sum = 0;
        for (int g = k + 1 + lane; g <= last_g; g += 64) sum += (int)gbl(D.gomc)[g];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (sum == 0) gt = (left + (last_g - k) / 2) / (last_g - k);
        else gt = (int)(uint32_t)(uint64_t)(((int64_t)(sum / 2) + (int64_t)(int32_t)gbl(D.gomc)[k + 1] * (int64_t)(uint32_t)left) / sum);
    }
    (void)G;
    if (lane < 4) gran_store(gs + 4 * k + lane, epoch, (uint32_t)(lane == 0 ? qp : lane == 1 ? fb : lane == 2 ? gt : last + 1));
    return qp;
}

// One workgroup per stream. (1) per-MB bit counts incl. mb_skip_run -> bit offsets (scans over
// contiguous MB ranges per thread); (2) slice header, MB bits and the stop bit OR-ed into the RBSP;
// (3) emulation prevention (7.4.1.1): a thread owns 64 consecutive RBSP bytes per 16 KiB chunk; the
// zero run before its first byte comes from a max-scan of the last non-zero byte position, its
// insertions from its own serial walk, its output offset from a sum-scan of the insertion counts;
// (4) the rate-control update of DESIGN.md §3.6 from the final NAL size.
// (the body of one stream's workgroup; enc_post_kernel runs it beside the reference planes, enc_planes.inc)
DEV void enc_pack_block(const PackLaunch &a, int stream) {
    __shared__ uint32_t s_hdr[8];
    __shared__ int s_hdrlen;
    __shared__ int s_w[PACK_WAVES];
    __shared__ int s_rb[256];     // macroblock_layer() bits per MB row (GOM rate control)
    __shared__ int s_rc[2];       // a frame was coded, mean row bits
    const int tid = threadIdx.x;
    const EncDesc &D = a.desc[stream];
    EncState *st = D.st;
    const bool inject_overflow = st->inject_err == 3;  // read by every thread before thread 0 clears it
    if (st->cur_skip) {  // frame skipped by the rate control (enc_begin_kernel): no output
        if (tid == 0) st->nal_bytes = 0;
        return;
    }
    const int nmb = a.mbw * a.mbh;
    const int idr = st->cur_idr, qp = st->cur_qp;
    uint32_t *rb = D.rbsp;
    for (int r = tid; r < a.mbh; r += PACK_THREADS) s_rb[r] = 0;
    // ---- slice header (7.3.3) into s_hdr
    if (tid == 0) {
        LBits b;
        lb_init(b, s_hdr);
        // OpenH264's slice header (WelsSliceHeaderWrite, h264.wasm func 1148; oracle h264o_enc_encode):
        // slice_type 2 / 0, 15-bit frame_num, no POC (type 2); P: num_ref_idx override to 1 active,
        // explicit reordering {idc 0, abs_diff_pic_num_minus1 0, idc 3}, marking flag 0; IDR: {0, 0}
        lb_ue(b, 0);
        lb_ue(b, idr ? 2 : 0);
        lb_ue(b, 0);
        lb_put(b, (uint32_t)st->frame_num, 15);
        if (idr) {
            lb_ue(b, (uint32_t)st->idr_pic_id);
            lb_put(b, 0, 2);
        } else {
            lb_put(b, 0x3, 2);      // num_ref_idx_active_override_flag 1, num_ref_idx_l0_active_minus1 ue(0)
            lb_put(b, 0x1C8, 9);    // ref_pic_list_modification_flag_l0 1, ue(0), ue(0), ue(3) = 00100,
                                    // adaptive_ref_pic_marking_mode_flag 0
        }
        lb_se(b, qp - 26);
        lb_ue(b, 0); lb_se(b, 0); lb_se(b, 0);
        lb_flush(b);
        s_hdrlen = b.total;
    }
    // ---- (1) contiguous MB range per thread (a multiple of 4 MBs): up to PACK_MBT lengths per thread
    // in registers from 16-byte loads (one round trip); larger pictures re-read the tail of the range
    constexpr int PACK_MBT = 32;
    const int per = ((nmb + PACK_THREADS - 1) / PACK_THREADS + 3) & ~3;
    const int i0 = min(nmb, tid * per), i1 = min(nmb, i0 + per);
    uint32_t Lr[PACK_MBT];
#pragma unroll
    for (int j = 0; j < PACK_MBT; j += 4) {
        u32x4 v = {0, 0, 0, 0};
        if (i0 + j + 3 < i1) v = *(const u32x4 *)(D.mblen + i0 + j);
        else if (i0 + j < i1) {
            v.x = D.mblen[i0 + j];
            if (i0 + j + 1 < i1) v.y = D.mblen[i0 + j + 1];
            if (i0 + j + 2 < i1) v.z = D.mblen[i0 + j + 2];
        }
        Lr[j] = v.x; Lr[j + 1] = v.y; Lr[j + 2] = v.z; Lr[j + 3] = v.w;
    }
    int my_last = -1;
#pragma unroll
    for (int j = 0; j < PACK_MBT; j++) if (Lr[j]) my_last = i0 + j;
    for (int i = i0 + PACK_MBT; i < i1; i++) if (D.mblen[i]) my_last = i;
    __syncthreads();  // s_rb cleared
    {   // row sums of the MB bit counts (mb_skip_run codes excluded), flushed at row changes
        int r = i0 < nmb ? i0 / a.mbw : 0, xe = (r + 1) * a.mbw, acc = 0;
        auto add = [&](int i, uint32_t l) {
            if (i >= xe) { if (acc) atomicAdd(&s_rb[r], acc); acc = 0; r++; xe += a.mbw; }
            acc += (int)l;
        };
#pragma unroll
        for (int j = 0; j < PACK_MBT; j++)  // constant indices into Lr: a variable one would put it in scratch
            if (i0 + j < i1) add(i0 + j, Lr[j]);
        for (int i = i0 + PACK_MBT; i < i1; i++) add(i, D.mblen[i]);
        if (acc) atomicAdd(&s_rb[r], acc);
    }
    int last_coded;
    const int prev = block_excl_scan<true>(my_last, s_w, &last_coded);  // last coded MB before i0
    int mybits = 0;
    {
        int p = prev;
#pragma unroll
        for (int j = 0; j < PACK_MBT; j++) {
            if (!Lr[j]) continue;
            mybits += (int)Lr[j] + (idr ? 0 : ue_len((uint32_t)(i0 + j - p - 1)));
            p = i0 + j;
        }
        for (int i = i0 + PACK_MBT; i < i1; i++) {
            const uint32_t l = D.mblen[i];
            if (!l) continue;
            mybits += (int)l + (idr ? 0 : ue_len((uint32_t)(i - p - 1)));
            p = i;
        }
    }
    int body;
    const int base = s_hdrlen + block_excl_scan<false>(mybits, s_w, &body);
    const int body_end = s_hdrlen + body;
    const int trail = idr ? 0 : nmb - 1 - last_coded;
    const int total_bits = body_end + (trail > 0 ? ue_len((uint32_t)trail) : 0) + 1;
    const int rbsp_bytes = (total_bits + 7) >> 3;
    const int nd = (rbsp_bytes + 3) >> 2;
    // RBSP overflow (or the test hook's code 3): the frame fails and publishes nothing -- the size word
    // every consumer reads (enc_fetch, copy_nals, ring_publish_kernel) becomes 0
    if (nd + 2 > D.rbsp_cap || inject_overflow) {
        if (tid == 0) { st->err = 2; st->nal_bytes = 0; st->inject_err = 0; }
        return;
    }
    for (int i = tid; i < nd + 2; i += PACK_THREADS) rb[i] = 0;
    __syncthreads();
    // ---- (2) RBSP bits: the first four dwords of 4 MBs of the range loaded together per batch (a P MB
    // rarely needs more than 128 bits); further dwords of longer MBs are loaded as they are reached
    {
        auto put_mb = [&](int i, uint32_t l, int pos, u32x4 a0) {
            const uint32_t *src = D.mbbits + (size_t)i * H264MI_MB_SLOT_DWORDS;
            const int n = (int)((l + 31) >> 5);
            for (int k = 0; k < n; k++) {
                const int nb = (k == n - 1 && (l & 31)) ? (int)(l & 31) : 32;
                const uint32_t v = k == 0 ? a0.x : k == 1 ? a0.y : k == 2 ? a0.z : k == 3 ? a0.w : src[k];
                bits_or(rb, pos + 32 * k, v >> (32 - nb), nb);
            }
        };
        int p = prev, pos = base;
#pragma unroll
        for (int j0 = 0; j0 < PACK_MBT; j0 += 4) {
            u32x4 w0[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
                w0[j] = Lr[j0 + j] ? *(const u32x4 *)(D.mbbits + (size_t)(i0 + j0 + j) * H264MI_MB_SLOT_DWORDS) : u32x4{0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t l = Lr[j0 + j];
                if (!l) continue;
                const int i = i0 + j0 + j;
                if (!idr) { const uint32_t run = (uint32_t)(i - p - 1); bits_ue(rb, pos, run); pos += ue_len(run); }
                put_mb(i, l, pos, w0[j]);
                pos += (int)l;
                p = i;
            }
        }
        for (int i = i0 + PACK_MBT; i < i1; i++) {
            const uint32_t l = D.mblen[i];
            if (!l) continue;
            if (!idr) { const uint32_t run = (uint32_t)(i - p - 1); bits_ue(rb, pos, run); pos += ue_len(run); }
            put_mb(i, l, pos, *(const u32x4 *)(D.mbbits + (size_t)i * H264MI_MB_SLOT_DWORDS));
            pos += (int)l;
            p = i;
        }
    }
    if (tid == 0) {
        const int nh = (s_hdrlen + 31) >> 5;
        for (int k = 0; k < nh; k++) {
            const int nb = (k == nh - 1 && (s_hdrlen & 31)) ? (s_hdrlen & 31) : 32;
            bits_or(rb, 32 * k, s_hdr[k] >> (32 - nb), nb);
        }
        int pos = body_end;
        if (trail > 0) { bits_ue(rb, pos, (uint32_t)trail); pos += ue_len((uint32_t)trail); }
        bits_or(rb, pos, 1, 1);  // rbsp_stop_one_bit
    }
    __syncthreads();
    // ---- (3) NAL assembly: [SPS PPS] + start code + header + EP(RBSP)
    uint8_t *out = D.nal;
    int hdr = 0;
    if (idr) {
        for (int i = tid; i < st->sps_bytes; i += PACK_THREADS) out[i] = st->sps[i];
        for (int i = tid; i < st->pps_bytes; i += PACK_THREADS) out[st->sps_bytes + i] = st->pps[i];
        hdr = st->sps_bytes + st->pps_bytes;
    }
    if (tid == 0) {
        out[hdr] = 0; out[hdr + 1] = 0; out[hdr + 2] = 0; out[hdr + 3] = 1;
        out[hdr + 4] = (uint8_t)((3 << 5) | (idr ? 5 : 1));
    }
    const int obase = hdr + 5;
    int carry_nz = -1, carry_ins = 0;  // over earlier chunks: last non-zero RBSP byte, insertions
    constexpr int EPB = 64;            // bytes per thread per chunk
    for (int c0 = 0; c0 < rbsp_bytes; c0 += EPB * PACK_THREADS) {
        const int b0 = c0 + EPB * tid;
        uint32_t wv[EPB / 4];
#pragma unroll
        for (int k = 0; k < EPB / 4; k++) {
            const int wi = (b0 >> 2) + k;
            wv[k] = b0 + 4 * k < rbsp_bytes ? __hip_atomic_load(&rb[wi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        }
        const int nb = max(0, min(EPB, rbsp_bytes - b0));
        int my_nz = -1;
#pragma unroll
        for (int k = 0; k < EPB; k++)
            if (k < nb && ((wv[k >> 2] >> (24 - 8 * (k & 3))) & 255)) my_nz = b0 + k;
        int chunk_nz, chunk_ins;
        const int pnz = max(carry_nz, block_excl_scan<true>(my_nz, s_w, &chunk_nz));
        // zeros immediately before b0 (the NAL header byte before the RBSP is non-zero)
        int z = pnz >= 0 ? b0 - 1 - pnz : b0;
        uint64_t insm = 0;  // bit k: insert 0x03 before byte k
        int z2 = z;
#pragma unroll
        for (int k = 0; k < EPB; k++) {
            const int byte = (int)((wv[k >> 2] >> (24 - 8 * (k & 3))) & 255);
            if (k < nb && byte <= 3 && z2 >= 2 && !(z2 & 1)) insm |= 1ull << k;
            z2 = byte == 0 ? z2 + 1 : 0;
        }
        const int my_ins = __popcll(insm);
        const int before = carry_ins + block_excl_scan<false>(my_ins, s_w, &chunk_ins);
        int o = obase + b0 + before;
        for (int k = 0; k < nb; k++) {
            if ((insm >> k) & 1) out[o++] = 3;
            out[o++] = (uint8_t)((wv[k >> 2] >> (24 - 8 * (k & 3))) & 255);
        }
        carry_nz = max(carry_nz, chunk_nz);
        carry_ins += chunk_ins;
    }
    // the average QPY of the coded macroblocks (RcUpdatePictureQpBits: iTotalQpSlice / iTotalMbSlice, func 1218):
    // a record flagged 0x80 is a non-carrier before its row's first carrier -- its QPY is the row's entry QP
    int sq_qp = 0, n_mb = 0;
    if (!idr) {
        int myq = 0, myn = 0;
        for (int i = i0; i < i1; i++) {
            if (!D.mblen[i]) continue;
            const uint32_t qb = (((const uint32_t *)D.info)[(size_t)i * 32] >> 8) & 0xffu;
            const int row = i / a.mbw;
            myq += (qb & 0x80u) ? (row == 0 ? qp : (int)(uint32_t)D.rowq[row]) : (int)qb;
            myn++;
        }
        (void)block_excl_scan<false>(myq, s_w, &sq_qp);
        (void)block_excl_scan<false>(myn, s_w, &n_mb);
    }
    __syncthreads();  // every thread is past reading st (the scans above), s_rb complete
    if (tid == 0) {
        if (st->inject_err) { st->err = st->inject_err; st->inject_err = 0; }  // test hook: as an RBSP overflow
        const int nbytes = obase + rbsp_bytes + carry_ins;
        // a failed frame publishes nothing: every consumer of the size word (enc_fetch, copy_nals,
        // ring_publish_kernel) sees 0 bytes, and the next frame is an IDR (enc_begin_kernel)
        st->nal_bytes = st->err ? 0 : nbytes;
        s_rc[0] = -1;
        if (!st->err) {  // a failed frame: no output (enc_fetch), no frame_num / POC / RC advance
            // WelsRcPictureInfoUpdateGom (func 1218; oracle rc_picture_update) on the slice NAL's bytes (the
            // parameter sets are another layer): the average QP, the R-Q model, the VGOP budget, the VBV skip check
            RcState &r = st->rc;
            const int bits = (nbytes - hdr) << 3;
            const int avg = (!idr && n_mb > 0) ? (n_mb * 50 + sq_qp * 100) / (n_mb * 100) : qp;
            r.last_qscale = avg;
            r.avg_qp = avg;
            if (!idr) {  // RcUpdateFrameComplexity (func 676)
                const int q = c_RC_QSTEP[avg];
                if (r.pframe_num == 0) {
                    r.frame_cmplx_mean = (int64_t)(int32_t)(uint32_t)(uint64_t)r.frame_cmplx;
                    r.linear_cmplx = (int64_t)bits * q;
                } else {
                    r.frame_cmplx_mean = (r.frame_cmplx * 20 + r.frame_cmplx_mean * 80 + 50) / 100;
                    r.linear_cmplx = (r.linear_cmplx * 80 + (int64_t)q * bits * 20 + 50) / 100;
                }
                r.pframe_num = (r.pframe_num >= 254 ? 254 : r.pframe_num) + 1;
            } else {     // RcUpdateIntraComplexity
                const int64_t ic = (int64_t)c_RC_QSTEP[avg] * bits;
                if (r.idr_num == 0) { r.intra_cmplx_mean = r.frame_cmplx; r.intra_cmplx = ic; }
                else {
                    r.intra_cmplx = (ic * 20 + r.intra_cmplx * 80 + 50) / 100;
                    r.intra_cmplx_mean = (r.frame_cmplx * 20 + r.intra_cmplx_mean * 80 + 50) / 100;
                }
                r.intra_mb_count = r.nmb;
                r.idr_num = (r.idr_num >= 254 ? 254 : r.idr_num) + 1;
            }
            r.remaining -= bits;
            if (r.skip_en) {  // RcVBufferCalculationSkip
#pragma clang fp contract(off)
                r.fullness += bits - r.bpf;
                int64_t pred = 0;
                if (r.frame_coded_in_vgop <= 6) pred = (int64_t)(7 - r.frame_coded_in_vgop) * r.min_bits_tl;
                const double inc = ((double)(pred - r.remaining) * 100.0) / (double)(r.bpf << 3) + -5.0;
                if ((r.fullness > r.buffer_size_skip && avg > r.skip_qp) || inc > 10.0) r.skip_flag = 1;
            }
            r.frame_coded_in_vgop++;
            st->frame_num = (st->frame_num + 1) & 0x7fff;
            st->poc += 2;
            int64_t sum = 0;
            for (int rr = 0; rr < a.mbh; rr++) sum += s_rb[rr];
            s_rc[0] = 1;
            s_rc[1] = (int)(sum / a.mbh);
        }
    }
    __syncthreads();
    // the next frame's MB-row QP plan (oracle rc_plan_rows / h264o_rc_row_delta)
    if (s_rc[0] >= 0) {
        const int mean = s_rc[1];
        for (int r = tid; r < a.mbh; r += PACK_THREADS) {
            const int b = s_rb[r];
            const int dr = mean <= 0 ? 0 : (b > 2 * mean ? 2 : (4 * (int64_t)b > 5 * (int64_t)mean ? 1 : (2 * b < mean ? -1 : 0)));
            D.rowbits[r] = b;
            D.rowqp[r] = dr;  // the row's offset; enc_mb_kernel clips frame QP + offset to the frame's window
        }
    }
}
// The same for a picture of more than one slice (DESIGN.md §3.7): the picture's slices one after the other, each
// through (1)-(3) into its own NAL unit. A function and a kernel of its own: the loop around the per-thread arrays
// costs registers (151 VGPRs against 117), which the single-slice pack above -- the default, kept as it was --
// must not pay (it has to fit beside the decoder's resident waves, see PACK_THREADS).
DEV void enc_pack_block_slices(const PackLaunch &a, int stream) {
    __shared__ uint32_t s_hdr[8];
    __shared__ int s_hdrlen;
    __shared__ int s_w[PACK_WAVES];
    __shared__ int s_rb[256];     // macroblock_layer() bits per MB row (GOM rate control)
    __shared__ int s_rc[2];       // a frame was coded, mean row bits
    const int tid = threadIdx.x;
    const EncDesc &D = a.desc[stream];
    EncState *st = D.st;
    const bool inject_overflow = st->inject_err == 3;  // read by every thread before thread 0 clears it
    if (st->cur_skip) {  // frame skipped by the rate control (enc_begin_kernel): no output
        if (tid == 0) st->nal_bytes = 0;
        return;
    }
    const int nmb = a.mbw * a.mbh;
    // (uniform values in SGPRs: the slice loop's control flow is then scalar, which keeps its registers down)
    const int idr = uni(st->cur_idr), qp = uni(st->cur_qp), nsl = uni(st->cur_slices);
    uint32_t *rb = D.rbsp;
    for (int r = tid; r < a.mbh; r += PACK_THREADS) s_rb[r] = 0;
    // the access unit: [SPS PPS] then the picture's nsl slice NAL units back to back (DESIGN.md §3.7), each with its
    // own header, mb_skip_run chain, stop bit, emulation prevention and start code; ooff: where the next one starts
    uint8_t *out = D.nal;
    int hdr = 0;
    if (idr) {
        for (int i = tid; i < st->sps_bytes; i += PACK_THREADS) out[i] = st->sps[i];
        for (int i = tid; i < st->pps_bytes; i += PACK_THREADS) out[st->sps_bytes + i] = st->pps[i];
        hdr = st->sps_bytes + st->pps_bytes;
    }
    int ooff = hdr;
    constexpr int PACK_MBT = 32;
#pragma unroll 1
    for (int sk = 0; sk < nsl; sk++) {
        // the slice's macroblocks [m0, m1): whole MB rows
        const int m0 = slice_first_row(a.mbh, nsl, sk) * a.mbw, m1 = slice_first_row(a.mbh, nsl, sk + 1) * a.mbw;
        // ---- slice header (7.3.3) into s_hdr
        if (tid == 0) {
            LBits b;
            lb_init(b, s_hdr);
            // OpenH264's slice header (WelsSliceHeaderWrite, h264.wasm func 1148; oracle h264o_enc_encode):
            // slice_type 2 / 0, 15-bit frame_num, no POC (type 2); P: num_ref_idx override to 1 active,
            // explicit reordering {idc 0, abs_diff_pic_num_minus1 0, idc 3}, marking flag 0; IDR: {0, 0}
            lb_ue(b, (uint32_t)m0);  // first_mb_in_slice
            lb_ue(b, idr ? 2 : 0);
            lb_ue(b, 0);
            lb_put(b, (uint32_t)st->frame_num, 15);
            if (idr) {
                lb_ue(b, (uint32_t)st->idr_pic_id);
                lb_put(b, 0, 2);
            } else {
                lb_put(b, 0x3, 2);      // num_ref_idx_active_override_flag 1, num_ref_idx_l0_active_minus1 ue(0)
                lb_put(b, 0x1C8, 9);    // ref_pic_list_modification_flag_l0 1, ue(0), ue(0), ue(3) = 00100,
                                        // adaptive_ref_pic_marking_mode_flag 0
            }
            lb_se(b, qp - 26);
            lb_ue(b, 0); lb_se(b, 0); lb_se(b, 0);
            lb_flush(b);
            s_hdrlen = b.total;
        }
        // ---- (1) contiguous MB range per thread (a multiple of 4 MBs): up to PACK_MBT lengths per thread
        // in registers from 16-byte loads (one round trip); larger pictures re-read the tail of the range.
        // The ranges are cut on a grid of 4 MBs from ib (the loads' alignment): thread 0's starts at m0, which
        // need not lie on it, so Lr[j] is MB ib + j and the entries outside [i0, i1) stay 0
        const int mg = m0 & ~3, per = ((m1 - mg + PACK_THREADS - 1) / PACK_THREADS + 3) & ~3;
        const int ib = mg + tid * per, i0 = min(m1, max(m0, ib)), i1 = max(i0, min(m1, ib + per));
        uint32_t Lr[PACK_MBT];
#pragma unroll
        for (int j = 0; j < PACK_MBT; j += 4) {
            u32x4 v = {0, 0, 0, 0};
            if (ib + j + 3 < i1) v = *(const u32x4 *)(D.mblen + ib + j);
            else if (ib + j < i1) {
                v.x = D.mblen[ib + j];
                if (ib + j + 1 < i1) v.y = D.mblen[ib + j + 1];
                if (ib + j + 2 < i1) v.z = D.mblen[ib + j + 2];
            }
            Lr[j] = v.x; Lr[j + 1] = v.y; Lr[j + 2] = v.z; Lr[j + 3] = v.w;
        }
        if (ib < i0) {  // the slice before this one ends inside the first group (i0 - ib <= 3)
            Lr[0] = 0;
            if (ib + 1 < i0) Lr[1] = 0;
            if (ib + 2 < i0) Lr[2] = 0;
        }
        int my_last = -1;
#pragma unroll
        for (int j = 0; j < PACK_MBT; j++) if (Lr[j]) my_last = ib + j;
        for (int i = ib + PACK_MBT; i < i1; i++) if (D.mblen[i]) my_last = i;
        __syncthreads();  // s_rb cleared, s_hdrlen of this slice written
        {   // row sums of the MB bit counts (mb_skip_run codes excluded), flushed at row changes
            int r = i0 < m1 ? i0 / a.mbw : 0, xe = (r + 1) * a.mbw, acc = 0;
            auto add = [&](int i, uint32_t l) {
                if (i >= xe) { if (acc) atomicAdd(&s_rb[r], acc); acc = 0; r++; xe += a.mbw; }
                acc += (int)l;
            };
#pragma unroll
            for (int j = 0; j < PACK_MBT; j++)  // constant indices into Lr: a variable one would put it in scratch
                if (ib + j < i1) add(ib + j, Lr[j]);  // (an entry before i0 is 0: it adds nothing)
            for (int i = ib + PACK_MBT; i < i1; i++) add(i, D.mblen[i]);
            if (acc) atomicAdd(&s_rb[r], acc);
        }
        // a skip run never crosses a slice edge: the slice's first run counts from m0, its trailing run ends at m1 - 1
        int last_coded;
        const int prev = max(m0 - 1, block_excl_scan<true>(my_last, s_w, &last_coded));  // last coded MB of the slice before i0
        last_coded = max(m0 - 1, last_coded);
        int mybits = 0;
        {
            int p = prev;
#pragma unroll
            for (int j = 0; j < PACK_MBT; j++) {
                if (!Lr[j]) continue;
                mybits += (int)Lr[j] + (idr ? 0 : ue_len((uint32_t)(ib + j - p - 1)));
                p = ib + j;
            }
            for (int i = ib + PACK_MBT; i < i1; i++) {
                const uint32_t l = D.mblen[i];
                if (!l) continue;
                mybits += (int)l + (idr ? 0 : ue_len((uint32_t)(i - p - 1)));
                p = i;
            }
        }
        int body;
        const int base = s_hdrlen + block_excl_scan<false>(mybits, s_w, &body);
        const int body_end = s_hdrlen + body;
        const int trail = idr ? 0 : m1 - 1 - last_coded;
        const int total_bits = uni(body_end + (trail > 0 ? ue_len((uint32_t)trail) : 0) + 1);
        const int rbsp_bytes = (total_bits + 7) >> 3;
        const int nd = (rbsp_bytes + 3) >> 2;
        // RBSP overflow, a NAL unit that may not fit the stream's NAL buffer behind the ones before it (at most one
        // emulation prevention byte per two RBSP bytes), or the test hook's code 3, in any slice: the whole frame fails
        // and publishes nothing -- the size word every consumer reads (enc_fetch, copy_nals, ring_publish_kernel) becomes 0
        if (nd + 2 > D.rbsp_cap || ooff + 5 + rbsp_bytes + (rbsp_bytes >> 1) + 1 > D.nal_cap || inject_overflow) {
            if (tid == 0) { st->err = 2; st->nal_bytes = 0; st->inject_err = 0; }
            return;
        }
        for (int i = tid; i < nd + 2; i += PACK_THREADS) rb[i] = 0;
        __syncthreads();
        // ---- (2) RBSP bits: the first four dwords of 4 MBs of the range loaded together per batch (a P MB
        // rarely needs more than 128 bits); further dwords of longer MBs are loaded as they are reached
        {
            auto put_mb = [&](int i, uint32_t l, int pos, u32x4 a0) {
                const uint32_t *src = D.mbbits + (size_t)i * H264MI_MB_SLOT_DWORDS;
                const int n = (int)((l + 31) >> 5);
                for (int k = 0; k < n; k++) {
                    const int nb = (k == n - 1 && (l & 31)) ? (int)(l & 31) : 32;
                    const uint32_t v = k == 0 ? a0.x : k == 1 ? a0.y : k == 2 ? a0.z : k == 3 ? a0.w : src[k];
                    bits_or(rb, pos + 32 * k, v >> (32 - nb), nb);
                }
            };
            int p = prev, pos = base;
#pragma unroll
            for (int j0 = 0; j0 < PACK_MBT; j0 += 4) {
                u32x4 w0[4];
#pragma unroll
                for (int j = 0; j < 4; j++)
                    w0[j] = Lr[j0 + j] ? *(const u32x4 *)(D.mbbits + (size_t)(ib + j0 + j) * H264MI_MB_SLOT_DWORDS) : u32x4{0, 0, 0, 0};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t l = Lr[j0 + j];
                    if (!l) continue;
                    const int i = ib + j0 + j;
                    if (!idr) { const uint32_t run = (uint32_t)(i - p - 1); bits_ue(rb, pos, run); pos += ue_len(run); }
                    put_mb(i, l, pos, w0[j]);
                    pos += (int)l;
                    p = i;
                }
            }
            for (int i = ib + PACK_MBT; i < i1; i++) {
                const uint32_t l = D.mblen[i];
                if (!l) continue;
                if (!idr) { const uint32_t run = (uint32_t)(i - p - 1); bits_ue(rb, pos, run); pos += ue_len(run); }
                put_mb(i, l, pos, *(const u32x4 *)(D.mbbits + (size_t)i * H264MI_MB_SLOT_DWORDS));
                pos += (int)l;
                p = i;
            }
        }
        if (tid == 0) {
            const int nh = (s_hdrlen + 31) >> 5;
            for (int k = 0; k < nh; k++) {
                const int nb = (k == nh - 1 && (s_hdrlen & 31)) ? (s_hdrlen & 31) : 32;
                bits_or(rb, 32 * k, s_hdr[k] >> (32 - nb), nb);
            }
            int pos = body_end;
            if (trail > 0) { bits_ue(rb, pos, (uint32_t)trail); pos += ue_len((uint32_t)trail); }
            bits_or(rb, pos, 1, 1);  // rbsp_stop_one_bit
        }
        __syncthreads();
        // ---- (3) NAL assembly at ooff: start code + header + EP(RBSP)
        if (tid == 0) {
            out[ooff] = 0; out[ooff + 1] = 0; out[ooff + 2] = 0; out[ooff + 3] = 1;
            out[ooff + 4] = (uint8_t)((3 << 5) | (idr ? 5 : 1));
        }
        const int obase = ooff + 5;
        int carry_nz = -1, carry_ins = 0;  // over earlier chunks: last non-zero RBSP byte, insertions
        constexpr int EPB = 64;            // bytes per thread per chunk
        for (int c0 = 0; c0 < rbsp_bytes; c0 += EPB * PACK_THREADS) {
            const int b0 = c0 + EPB * tid;
            uint32_t wv[EPB / 4];
#pragma unroll
            for (int k = 0; k < EPB / 4; k++) {
                const int wi = (b0 >> 2) + k;
                wv[k] = b0 + 4 * k < rbsp_bytes ? __hip_atomic_load(&rb[wi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            }
            const int nb = max(0, min(EPB, rbsp_bytes - b0));
            int my_nz = -1;
#pragma unroll
            for (int k = 0; k < EPB; k++)
                if (k < nb && ((wv[k >> 2] >> (24 - 8 * (k & 3))) & 255)) my_nz = b0 + k;
            int chunk_nz, chunk_ins;
            const int pnz = max(carry_nz, block_excl_scan<true>(my_nz, s_w, &chunk_nz));
            // zeros immediately before b0 (the NAL header byte before the RBSP is non-zero)
            int z = pnz >= 0 ? b0 - 1 - pnz : b0;
            uint64_t insm = 0;  // bit k: insert 0x03 before byte k
            int z2 = z;
#pragma unroll
            for (int k = 0; k < EPB; k++) {
                const int byte = (int)((wv[k >> 2] >> (24 - 8 * (k & 3))) & 255);
                if (k < nb && byte <= 3 && z2 >= 2 && !(z2 & 1)) insm |= 1ull << k;
                z2 = byte == 0 ? z2 + 1 : 0;
            }
            const int my_ins = __popcll(insm);
            const int before = carry_ins + block_excl_scan<false>(my_ins, s_w, &chunk_ins);
            int o = obase + b0 + before;
            for (int k = 0; k < nb; k++) {
                if ((insm >> k) & 1) out[o++] = 3;
                out[o++] = (uint8_t)((wv[k >> 2] >> (24 - 8 * (k & 3))) & 255);
            }
            carry_nz = max(carry_nz, chunk_nz);
            carry_ins += chunk_ins;
        }
        // the next slice's NAL unit follows this one; its RBSP reuses rb (every thread has loaded its bytes of this one
        // before the scans above, and zeroes rb only behind the next slice's)
        ooff = uni(obase + rbsp_bytes + carry_ins);
    }
    // the average QPY of the coded macroblocks (RcUpdatePictureQpBits: iTotalQpSlice / iTotalMbSlice, func 1218):
    // a record flagged 0x80 is a non-carrier before its row's first carrier -- its QPY is the row's entry QP,
    // the slice QP in a slice's first row
    int sq_qp = 0, n_mb = 0;
    if (!idr) {
        const int per = ((nmb + PACK_THREADS - 1) / PACK_THREADS + 3) & ~3, i0 = min(nmb, tid * per), i1 = min(nmb, i0 + per);
        int myq = 0, myn = 0;
        for (int i = i0; i < i1; i++) {
            if (!D.mblen[i]) continue;
            const uint32_t qb = (((const uint32_t *)D.info)[(size_t)i * 32] >> 8) & 0xffu;
            const int row = i / a.mbw;
            myq += (qb & 0x80u) ? ((row == 0 || (nsl > 1 && slice_row_first(a.mbh, nsl, row))) ? qp : (int)(uint32_t)D.rowq[row]) : (int)qb;
            myn++;
        }
        (void)block_excl_scan<false>(myq, s_w, &sq_qp);
        (void)block_excl_scan<false>(myn, s_w, &n_mb);
    }
    __syncthreads();  // every thread is past reading st (the scans above), s_rb complete
    if (tid == 0) {
        if (st->inject_err) { st->err = st->inject_err; st->inject_err = 0; }  // test hook: as an RBSP overflow
        const int nbytes = ooff;  // parameter sets + every slice NAL unit
        // a failed frame publishes nothing: every consumer of the size word (enc_fetch, copy_nals,
        // ring_publish_kernel) sees 0 bytes, and the next frame is an IDR (enc_begin_kernel)
        st->nal_bytes = st->err ? 0 : nbytes;
        s_rc[0] = -1;
        if (!st->err) {  // a failed frame: no output (enc_fetch), no frame_num / POC / RC advance
            // WelsRcPictureInfoUpdateGom (func 1218; oracle rc_picture_update) on the slice NAL's bytes (the
            // parameter sets are another layer): the average QP, the R-Q model, the VGOP budget, the VBV skip check
            RcState &r = st->rc;
            const int bits = (nbytes - hdr) << 3;
            const int avg = (!idr && n_mb > 0) ? (n_mb * 50 + sq_qp * 100) / (n_mb * 100) : qp;
            r.last_qscale = avg;
            r.avg_qp = avg;
            if (!idr) {  // RcUpdateFrameComplexity (func 676)
                const int q = c_RC_QSTEP[avg];
                if (r.pframe_num == 0) {
                    r.frame_cmplx_mean = (int64_t)(int32_t)(uint32_t)(uint64_t)r.frame_cmplx;
                    r.linear_cmplx = (int64_t)bits * q;
                } else {
                    r.frame_cmplx_mean = (r.frame_cmplx * 20 + r.frame_cmplx_mean * 80 + 50) / 100;
                    r.linear_cmplx = (r.linear_cmplx * 80 + (int64_t)q * bits * 20 + 50) / 100;
                }
                r.pframe_num = (r.pframe_num >= 254 ? 254 : r.pframe_num) + 1;
            } else {     // RcUpdateIntraComplexity
                const int64_t ic = (int64_t)c_RC_QSTEP[avg] * bits;
                if (r.idr_num == 0) { r.intra_cmplx_mean = r.frame_cmplx; r.intra_cmplx = ic; }
                else {
                    r.intra_cmplx = (ic * 20 + r.intra_cmplx * 80 + 50) / 100;
                    r.intra_cmplx_mean = (r.frame_cmplx * 20 + r.intra_cmplx_mean * 80 + 50) / 100;
                }
                r.intra_mb_count = r.nmb;
                r.idr_num = (r.idr_num >= 254 ? 254 : r.idr_num) + 1;
            }
            r.remaining -= bits;
            if (r.skip_en) {  // RcVBufferCalculationSkip
#pragma clang fp contract(off)
                r.fullness += bits - r.bpf;
                int64_t pred = 0;
                if (r.frame_coded_in_vgop <= 6) pred = (int64_t)(7 - r.frame_coded_in_vgop) * r.min_bits_tl;
                const double inc = ((double)(pred - r.remaining) * 100.0) / (double)(r.bpf << 3) + -5.0;
                if ((r.fullness > r.buffer_size_skip && avg > r.skip_qp) || inc > 10.0) r.skip_flag = 1;
            }
            r.frame_coded_in_vgop++;
            st->frame_num = (st->frame_num + 1) & 0x7fff;
            st->poc += 2;
            int64_t sum = 0;
            for (int rr = 0; rr < a.mbh; rr++) sum += s_rb[rr];
            s_rc[0] = 1;
            s_rc[1] = (int)(sum / a.mbh);
        }
    }
    __syncthreads();
    // the next frame's MB-row QP plan (oracle rc_plan_rows / h264o_rc_row_delta)
    if (s_rc[0] >= 0) {
        const int mean = s_rc[1];
        for (int r = tid; r < a.mbh; r += PACK_THREADS) {
            const int b = s_rb[r];
            const int dr = mean <= 0 ? 0 : (b > 2 * mean ? 2 : (4 * (int64_t)b > 5 * (int64_t)mean ? 1 : (2 * b < mean ? -1 : 0)));
            D.rowbits[r] = b;
            D.rowqp[r] = dr;  // the row's offset; enc_mb_kernel clips frame QP + offset to the frame's window
        }
    }
}
__global__ __launch_bounds__(PACK_THREADS) void enc_pack_kernel(PackLaunch a) { enc_pack_block(a, blockIdx.x); }
__global__ __launch_bounds__(PACK_THREADS) void enc_pack_slices_kernel(PackLaunch a) { enc_pack_block_slices(a, blockIdx.x); }

}  // namespace h264mi
