// deblock.inc -- H.264 loop filter (8.7) as an MB-row wavefront (gfx950).
//
// Replaces the loop filter inside OpenH264's encoder (reference for the next P frame) and
// decoder (output picture) behind openh264_wrapper.cpp:384 / :435. The filter is order
// dependent (MB raster order, vertical edges before horizontal), which allows exactly the same
// 2-MB-lag wavefront as intra prediction: MB (x,y) is filtered after (x+1,y-1). One wave per
// (stream, MB row). The row above hands over its bottom rows (luma 12..15, chroma 6..7, final
// except for this row's top edge) as {epoch,payload} granules; this row writes rows 13..15 of the
// MB above after filtering its top edge. Lane-per-line filtering out of a 20x20 (luma) /
// 10x10 (chroma) LDS working tile.
namespace h264mi {

constexpr uint8_t DBK_ALPHA[52] = {0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,   0,   0,   0,   0,   0,   4,   4,
                                          5,  6,  7,  8,  9,  10, 12, 13, 15, 17, 20,  22,  25,  28,  32,  36,  40,  45,
                                          50, 56, 63, 71, 80, 90, 101, 113, 127, 144, 162, 182, 203, 226, 255, 255};
constexpr uint8_t DBK_BETA[52] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4,
                                         6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17, 18, 18};
constexpr uint8_t DBK_TC0[52][3] = {
    {0, 0, 0},  {0, 0, 0},  {0, 0, 0},   {0, 0, 0},   {0, 0, 0},   {0, 0, 0},   {0, 0, 0},   {0, 0, 0},   {0, 0, 0},
    {0, 0, 0},  {0, 0, 0},  {0, 0, 0},   {0, 0, 0},   {0, 0, 0},   {0, 0, 0},   {0, 0, 0},   {0, 0, 0},   {0, 0, 1},
    {0, 0, 1},  {0, 0, 1},  {0, 0, 1},   {0, 1, 1},   {0, 1, 1},   {1, 1, 1},   {1, 1, 1},   {1, 1, 1},   {1, 1, 1},
    {1, 1, 2},  {1, 1, 2},  {1, 1, 2},   {1, 1, 2},   {1, 2, 3},   {1, 2, 3},   {2, 2, 3},   {2, 2, 4},   {2, 3, 4},
    {2, 3, 4},  {3, 3, 5},  {3, 4, 6},   {3, 4, 6},   {4, 5, 7},   {4, 5, 8},   {4, 6, 9},   {5, 7, 10},  {6, 8, 11},
    {6, 8, 13}, {7, 10, 14}, {8, 11, 16}, {9, 12, 18}, {10, 13, 20}, {11, 15, 23}, {13, 17, 25}};

// The same tables as dwords, so that a wave-uniform index is one scalar load (byte tables compile to
// per-lane vector byte loads): indexA -> alpha | tC0[0] << 8 | tC0[1] << 16 | tC0[2] << 24, indexB -> beta.
struct DbkTabs { uint32_t a[52], b[52]; };
constexpr DbkTabs build_dbk_tabs() {
    DbkTabs t{};
    for (int i = 0; i < 52; i++) {
        t.a[i] = DBK_ALPHA[i] | (uint32_t)DBK_TC0[i][0] << 8 | (uint32_t)DBK_TC0[i][1] << 16 | (uint32_t)DBK_TC0[i][2] << 24;
        t.b[i] = DBK_BETA[i];
    }
    return t;
}
__constant__ const DbkTabs c_DBK = build_dbk_tabs();

struct DbkDesc {
    const uint8_t *rec[3];  // unfiltered picture (coded size)
    uint8_t *out[2][3];     // filtered output (coded size), chosen by *parity (out[0] if parity == nullptr)
    const MbInfo *info;
    uint64_t *dgran;
    const uint32_t *epoch;
    const int32_t *disable; // nullptr, or the slice deblocking word: idc (1 -> no filtering) | offsets (see deblock_row)
    const int32_t *active;  // nullptr or nonzero -> run (decoder: a picture was parsed)
    const int32_t *parity;
    int32_t *abort_word;
    const uint64_t *src_gran;  // encoder: the MB wavefront hands each MB's unfiltered samples and record
                               // over as 128 granules (luma 0..63, chroma 64..95, MbInfo 96..127)
};
struct DbkOut {
    GLOBAL uint8_t *dbk[3];
    // chroma plane pl (per lane) by integer select: an indexed dbk[1 + pl] would put the struct in scratch
    DEV GLOBAL uint8_t *chroma(int pl) const {
        const uint64_t c1 = (uint64_t)dbk[1], dc = (uint64_t)dbk[2] - c1;
        return (GLOBAL uint8_t *)(c1 + (pl ? dc : 0));
    }
};
struct DbkLaunch { int mbw, mbh, S; const DbkDesc *desc; uint32_t *ticket; uint64_t *prof = nullptr; };  // prof: 16 section cycle totals

struct DbkLds {
    alignas(16) uint8_t L[20 * 20];        // luma tile rows/cols -4..15 relative to the current MB
    alignas(16) uint8_t C[2][10 * 12];     // chroma tiles rows -2..7, cols -4..7 (-2..-1 used)
    alignas(16) uint8_t prev[256];
    alignas(16) uint8_t prevc[2][64];  // previous MB (x-1), filtered except rows 13..15 (row below)
    int bs[2][4][4];           // [dir][edge][segment]
    alignas(16) MbInfo cur;
    alignas(16) MbInfo left;
    alignas(16) MbInfo top;
};

DEV void filt(uint8_t *q, int st, int bS, int alpha, int beta, int tc0, int chroma) {
    int p0 = q[-st], p1 = q[-2 * st], q0 = q[0], q1 = q[st];
    if (!(iabs(p0 - q0) < alpha && iabs(p1 - p0) < beta && iabs(q1 - q0) < beta)) return;
    if (bS < 4) {
        if (chroma) {
            int tc = tc0 + 1;
            int d = clip3(-tc, tc, (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3);
            q[-st] = (uint8_t)clip1(p0 + d); q[0] = (uint8_t)clip1(q0 - d);
        } else {
            int p2 = q[-3 * st], q2 = q[2 * st];
            int ap = iabs(p2 - p0), aq = iabs(q2 - q0);
            int tc = tc0 + (ap < beta) + (aq < beta);
            int d = clip3(-tc, tc, (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3);
            q[-st] = (uint8_t)clip1(p0 + d); q[0] = (uint8_t)clip1(q0 - d);
            if (ap < beta) q[-2 * st] = (uint8_t)(p1 + clip3(-tc0, tc0, (p2 + ((p0 + q0 + 1) >> 1) - (p1 << 1)) >> 1));
            if (aq < beta) q[st] = (uint8_t)(q1 + clip3(-tc0, tc0, (q2 + ((p0 + q0 + 1) >> 1) - (q1 << 1)) >> 1));
        }
    } else {
        if (chroma) {
            q[-st] = (uint8_t)((2 * p1 + p0 + q1 + 2) >> 2);
            q[0] = (uint8_t)((2 * q1 + q0 + p1 + 2) >> 2);
        } else {
            int p2 = q[-3 * st], q2 = q[2 * st], p3 = q[-4 * st], q3 = q[3 * st];
            int ap = iabs(p2 - p0), aq = iabs(q2 - q0);
            bool small = iabs(p0 - q0) < ((alpha >> 2) + 2);
            if (ap < beta && small) {
                q[-st] = (uint8_t)((p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3);
                q[-2 * st] = (uint8_t)((p2 + p1 + p0 + q0 + 2) >> 2);
                q[-3 * st] = (uint8_t)((2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3);
            } else q[-st] = (uint8_t)((2 * p1 + p0 + q1 + 2) >> 2);
            if (aq < beta && small) {
                q[0] = (uint8_t)((p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3);
                q[st] = (uint8_t)((p0 + q0 + q1 + q2 + 2) >> 2);
                q[2 * st] = (uint8_t)((2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3);
            } else q[0] = (uint8_t)((2 * q1 + q0 + p1 + 2) >> 2);
        }
    }
}
// 8.7.2.3 / 8.7.2.4 on one line held in registers: v[o..o+7] = p3 p2 p1 p0 q0 q1 q2 q3. Branch-free
// (luma and chroma lanes run the same instruction stream); b == 0 leaves the line unchanged. STRONG:
// the edge can have bS 4 (a macroblock edge); internal edges (bS <= 3) skip the strong filter's work.
template <bool STRONG>
DEV void filt_reg(int *v, int b, int alpha, int beta, int tc0, bool chroma) {
    const int p3 = v[0], p2 = v[1], p1 = v[2], p0 = v[3], q0 = v[4], q1 = v[5], q2 = v[6], q3 = v[7];
    const bool on = b != 0 && iabs(p0 - q0) < alpha && iabs(p1 - p0) < beta && iabs(q1 - q0) < beta;
    const bool apb = iabs(p2 - p0) < beta && !chroma, aqb = iabs(q2 - q0) < beta && !chroma;
    // bS < 4
    const int tc = chroma ? tc0 + 1 : tc0 + apb + aqb;
    const int d = clip3(-tc, tc, (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3);
    const int w0p = clip1(p0 + d), w0q = clip1(q0 - d);
    const int avg = (p0 + q0 + 1) >> 1;
    const int w1p = apb ? p1 + clip3(-tc0, tc0, (p2 + avg - (p1 << 1)) >> 1) : p1;
    const int w1q = aqb ? q1 + clip3(-tc0, tc0, (q2 + avg - (q1 << 1)) >> 1) : q1;
    if constexpr (!STRONG) {
        if (on) { v[3] = w0p; v[4] = w0q; v[2] = w1p; v[5] = w1q; }
        return;
    }
    // bS == 4
    const bool small = iabs(p0 - q0) < ((alpha >> 2) + 2);
    const bool sp = apb && small, sq = aqb && small;
    const int s0p = sp ? (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3 : (2 * p1 + p0 + q1 + 2) >> 2;
    const int s1p = sp ? (p2 + p1 + p0 + q0 + 2) >> 2 : p1;
    const int s2p = sp ? (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3 : p2;
    const int s0q = sq ? (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3 : (2 * q1 + q0 + p1 + 2) >> 2;
    const int s1q = sq ? (p0 + q0 + q1 + q2 + 2) >> 2 : q1;
    const int s2q = sq ? (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3 : q2;
    const bool strong = b == 4;
    if (on) {
        v[3] = strong ? s0p : w0p; v[4] = strong ? s0q : w0q;
        v[2] = strong ? s1p : w1p; v[5] = strong ? s1q : w1q;
        v[1] = strong ? s2p : p2;  v[6] = strong ? s2q : q2;
    }
}
DEV bool mbi_intra(int t) { return t == MI_I4 || t == MI_I16 || t == MI_IPCM; }
// Branch-free: every field is read up front (independent LDS loads, one wait) and the rules of
// 8.7.2.1 are applied as selects -- the lanes of a wave take different rules, so an early-return form
// runs every path with EXEC masking and serialises its loads behind the branches.
DEV int bs_of(const MbInfo &p, int rp, const MbInfo &q, int rq, bool mbedge) {  // 8.7.2.1
    const int tp = p.type, tq = q.type;
    const int np = p.nnz[rp], nq = q.nnz[rq];
    const int refp = p.ref[((rp >> 3) << 1) | ((rp & 3) >> 1)], refq = q.ref[((rq >> 3) << 1) | ((rq & 3) >> 1)];
    const uint32_t mp = *(const uint32_t *)&p.mv[rp][0], mq = *(const uint32_t *)&q.mv[rq][0];
    const int dx = (int)(int16_t)(mp & 0xffffu) - (int)(int16_t)(mq & 0xffffu);
    const int dy = (int)(int16_t)(mp >> 16) - (int)(int16_t)(mq >> 16);
    const bool intra = mbi_intra(tp) || mbi_intra(tq);
    const bool motion = refp != refq || iabs(dx) >= 4 || iabs(dy) >= 4;
    const int b = (np | nq) ? 2 : (motion ? 1 : 0);
    return intra ? (mbedge ? 4 : 3) : b;
}
DEV int qp_dbk(const MbInfo &m) { return m.type == MI_IPCM ? 0 : m.qp; }
// I_PCM: QPY = 0 for the filter (8.7.2.2); its chroma QP is that of QPY 0 + chroma_qp_index_offset,
// which the parser already stored in qpc
DEV int qpc_dbk(const MbInfo &m) { return m.qpc; }

DEV void dbk_flush(const DbkLds &S, const DbkOut &D, GLOBAL uint64_t *grow, uint32_t epoch, int mbx, int mby, int cw,
                   bool last_row) {
    // MB (mbx, mby) held in S.prev is final for this row: rows 0..12 luma / 0..6 chroma (all rows on
    // the last MB row) go to the picture; rows 12..15 / 6..7 go to the row below as granules.
    const int lane = threadIdx.x, ccw = cw / 2;
    {
        int r = lane >> 2, c4 = (lane & 3) * 4;
        if (r <= 12 || last_row)
            *(GLOBAL uint32_t *)&D.dbk[0][(size_t)(mby * 16 + r) * cw + mbx * 16 + c4] = *(const uint32_t *)&S.prev[r * 16 + c4];
    }
    if (lane < 32) {
        int pl = lane >> 4, r = (lane >> 1) & 7, hh = lane & 1;
        if (r <= 6 || last_row)
            *(GLOBAL uint32_t *)&D.chroma(pl)[(size_t)(mby * 8 + r) * ccw + mbx * 8 + hh * 4] = *(const uint32_t *)&S.prevc[pl][r * 8 + hh * 4];
    }
    if (!last_row && lane < 24) {
        uint32_t v = lane < 16 ? ((const uint32_t *)S.prev)[48 + lane] : ((const uint32_t *)S.prevc[(lane - 16) >> 2])[12 + ((lane - 16) & 3)];
        gran_store(grow + (size_t)mbx * H264MI_DBK_GRANULES_PER_MB + lane, epoch, v);
    }
}

// Per-edge filter strength parameters (8.7.2.2): alpha, beta and the three tC0 of one averaged QP,
// read with a uniform index (scalar loads).
// indexA = qPav + FilterOffsetA, indexB = qPav + FilterOffsetB (8-460, 8-461), both clipped to 0..51.
struct EdgeQ { int alpha, beta, t1, t2, t3; };
DEV EdgeQ edge_q(int qpav, int off_a, int off_b) {
    const int ia = uni(clip3(0, 51, qpav + off_a)), ib = uni(clip3(0, 51, qpav + off_b));
    const uint32_t ea = uni(c_DBK.a[ia]), eb = uni(c_DBK.b[ib]);
    return EdgeQ{(int)(ea & 255u), (int)eb, (int)((ea >> 8) & 255u), (int)((ea >> 16) & 255u), (int)(ea >> 24)};
}

// Sources of the unfiltered MB tile and MB records, lane-wise (lane: luma dword lane = row lane >> 2,
// columns (lane & 3) * 4; lanes 0..31: chroma dword (plane lane >> 4, row (lane >> 1) & 7, half
// lane & 1) and this MB's record dword; lanes 32..63: the record dword lane - 32 of the MB above).
// Global: the picture and records were written by an earlier launch -> loaded one MB ahead.
struct DbkSrcGlobal {
    GLOBAL const uint8_t *rec0, *rec1, *rec2;
    GLOBAL const uint32_t *info32;
    int cw, mbw, mby;
    uint32_t pl = 0, pc = 0, pi = 0;
    DEV void issue(int mx) {
        const int lane = threadIdx.x & 63, ccw = cw / 2;
        pl = *(GLOBAL const uint32_t *)&rec0[(size_t)(mby * 16 + (lane >> 2)) * cw + mx * 16 + (lane & 3) * 4];
        if (lane < 32) {
            const int c = lane >> 4, r = (lane >> 1) & 7, hh = lane & 1;
            pc = *(GLOBAL const uint32_t *)&(c ? rec2 : rec1)[(size_t)(mby * 8 + r) * ccw + mx * 8 + hh * 4];
            pi = info32[(size_t)(mby * mbw + mx) * 32 + lane];
        } else if (mby > 0) pi = info32[(size_t)((mby - 1) * mbw + mx) * 32 + lane - 32];
    }
    DEV void start() { issue(0); }
    DEV bool get(int mx, uint32_t &l, uint32_t &c, uint32_t &i, int32_t *) {
        l = pl; c = pc; i = pi;
        if (mx + 1 < mbw) issue(mx + 1);
        return true;
    }
};
// Granules: the MB wavefront of the same launch publishes them as it goes; a bounded sweep waits.
struct DbkSrcGranules {
    GLOBAL const uint64_t *g;  // stream's granule array (128 per MB)
    int mbw, mby;
    uint32_t epoch;
    GLOBAL const uint64_t *rowq;  // QPY entering each MB row (row_entry_qp), for records flagged 0x80
    int slice_qp;
    // row mby / mby - 1 is its slice's first row: entered at the slice QP (row_entry_qp). Only the encoder's records
    // are ever flagged 0x80 (a decoder's QP byte is at most 51), so the decoder, which leaves rowq null, never gets
    // there; the default keeps even such a record off rowq
    bool first_c = true, first_t = true;
    uint64_t xl, xc, xi;       // the granules of the MB get() is asked for next, loaded one MB ahead
    // loads of MB mx's granules (tile dword `lane`, chroma, records of MB mx and the MB above); their
    // values are consumed by the next get(), so the load latency overlaps the current MB's filtering
    DEV void issue(int mx) {
        const int lane = threadIdx.x & 63;
        GLOBAL const uint64_t *m = g + (size_t)(mby * mbw + mx) * 128;
        GLOBAL const uint64_t *gi = lane < 32 ? m + 96 + lane : (mby > 0 ? m - (size_t)mbw * 128 + 96 + lane - 32 : nullptr);
        xl = __hip_atomic_load(m + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        xc = lane < 32 ? __hip_atomic_load(m + 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ((uint64_t)epoch << 32);
        xi = gi ? __hip_atomic_load(gi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ((uint64_t)epoch << 32);
    }
    DEV void start() { issue(0); }
    DEV bool resolve_qp(uint32_t &i, int32_t *abort_word) const;
    DEV bool get(int mx, uint32_t &l, uint32_t &c, uint32_t &i, int32_t *abort_word) {
        WaitClock wc;
        for (unsigned spins = 0;; spins++) {
            l = (uint32_t)xl; c = (uint32_t)xc; i = (uint32_t)xi;
            const bool sl = (uint32_t)(xl >> 32) != epoch, sc = (uint32_t)(xc >> 32) != epoch, si = (uint32_t)(xi >> 32) != epoch;
            const uint64_t bad = __ballot(sl || sc || si);
            if (bad == 0) {
                const bool ok = resolve_qp(i, abort_word);
                if (mx + 1 < mbw) issue(mx + 1);
                return ok;
            }
#if !H264MI_GRAN_WAIT1
            if ((spins & 255) == 255) {
                const int ab = __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (ab || wc.expired()) {
                    if ((threadIdx.x & 63) == 0) __hip_atomic_store(abort_word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    return false;
                }
            }
            __builtin_amdgcn_s_sleep(1);
            issue(mx);
            continue;
#endif
            // stale: wait on the first stale granule alone (one 8-byte poll, not the MB's 160 granule loads), then
            // reload the MB's set
            const int k = (int)__builtin_ctzll(bad);
            GLOBAL const uint64_t *m = g + (size_t)(mby * mbw + mx) * 128;
            const int kl = __builtin_amdgcn_readlane((int)sl, k), kc = __builtin_amdgcn_readlane((int)sc, k);
            GLOBAL const uint64_t *p = kl ? m + k : kc ? m + 64 + k : (k < 32 ? m + 96 + k : m - (size_t)mbw * 128 + 96 + k - 32);
            if (!gran_wait1(p, epoch, abort_word, spins, wc)) return false;
            issue(mx);
        }
    }
};

// Encoder records whose QPY is the QP entering their row (DESIGN.md §3.6: no mb_qp_delta carrier
// before them in the row; QP and QPc bytes flagged 0x80): substitute it. Lanes 0/1 hold dwords 0/1
// (type|qp|.., cmode|qpc) of this MB, lanes 32/33 those of the MB above.
DEV bool DbkSrcGranules::resolve_qp(uint32_t &i, int32_t *abort_word) const {
    const int lane = threadIdx.x & 63;
    const uint32_t q0 = (uint32_t)__builtin_amdgcn_readlane((int)i, 0), t0 = (uint32_t)__builtin_amdgcn_readlane((int)i, 32);
    const bool pc = (q0 >> 8) & 0x80u, pt = mby > 0 && ((t0 >> 8) & 0x80u);
    int ec = 0, et = 0;
    if (pc && !row_entry_qp(rowq, mby, first_c, slice_qp, epoch, abort_word, &ec)) return false;
    if (pt && !row_entry_qp(rowq, mby - 1, first_t, slice_qp, epoch, abort_word, &et)) return false;
    const bool mine = lane < 32 ? pc : pt;
    const int e = lane < 32 ? ec : et;
    if (mine && (lane & 31) == 0) i = (i & ~0xff00u) | ((uint32_t)e << 8);
    if (mine && (lane & 31) == 1) i = (i & ~0xff00u) | ((uint32_t)c_CHROMA_QP[e] << 8);
    return true;
}

// One MB row of one stream (one wave): MB (x, y) is filtered after (x+1, y-1) (2-MB-lag wavefront).
template <class Src>
DEV void deblock_row(DbkLds &S, const DbkLaunch &a, CONSTANT const DbkDesc &DD, int mby, Src src) {
    const int lane = threadIdx.x & 63;
    if (DD.active && uni(*DD.active) == 0) return;
    const int par = DD.parity ? (uni(*DD.parity) & 1) : 0;
    const DbkOut D{{gbl(DD.out[par][0]), gbl(DD.out[par][1]), gbl(DD.out[par][2])}};
    const uint32_t epoch = (uint32_t)uni((int)*DD.epoch);
    // loop-filter parameters per MB, from its record's slice word (dword 31, h264mi_types.h MB_SLICE_*:
    // its slice's first MB, disable_deblocking_filter_idc, FilterOffsetA / B); 0 for the encoder's records
    const int mbw = a.mbw, cw = mbw * 16, ccw = cw / 2;
    const bool last_row = mby == a.mbh - 1;
    GLOBAL uint64_t *gprev = gbl(DD.dgran) + (size_t)(mby > 0 ? mby - 1 : 0) * mbw * H264MI_DBK_GRANULES_PER_MB;
    GLOBAL uint64_t *grow = gbl(DD.dgran) + (size_t)mby * mbw * H264MI_DBK_GRANULES_PER_MB;
    const int Y = mby * 16;
    src.start();
    // section timer (diagnostic, a.prof): 1 tile+prefetch, 2 top hand-off wait, 3 bS + edge params,
    // 4 filtering, 5 stores + flush
    uint64_t t_prev = a.prof ? clock64() : 0, s_prof[6] = {0, 0, 0, 0, 0, 0};
    auto lap = [&](int k) { if (a.prof) { const uint64_t tt = clock64(); s_prof[k] += tt - t_prev; t_prev = tt; } };

    int left_qp = 0, left_qpc = 0;  // the left MB's filter QPs (qp_dbk / qpc_dbk)
    for (int mbx = 0; mbx < mbw; mbx++) {
        const int X = mbx * 16;
        // ---- this MB's working tile (unfiltered) and records
        uint32_t pf_l, pf_c, pf_i;
        if (!src.get(mbx, pf_l, pf_c, pf_i, DD.abort_word)) return;
        *(uint32_t *)&S.L[((lane >> 2) + 4) * 20 + 4 + (lane & 3) * 4] = pf_l;
        if (lane < 32) {
            const int pl = lane >> 4, r = (lane >> 1) & 7, hh = lane & 1;
            *(uint32_t *)&S.C[pl][(r + 2) * 12 + 4 + hh * 4] = pf_c;
            ((uint32_t *)&S.cur)[lane] = pf_i;
        } else if (mby > 0) ((uint32_t *)&S.top)[lane - 32] = pf_i;
        // ---- left margin: MB x-1 cols 12..15 (filtered except its rows 13..15 by the row below)
        if (mbx > 0) {
            { int r = lane >> 2, c = lane & 3; S.L[(r + 4) * 20 + c] = S.prev[r * 16 + 12 + c]; }
            if (lane < 32) { int pl = lane >> 4, r = (lane >> 1) & 7, c = lane & 1; S.C[pl][(r + 2) * 12 + 2 + c] = S.prevc[pl][r * 8 + 6 + c]; }
        }
        lap(1);
        // ---- top margin: MB (x, y-1) rows 12..15, final after (x+1, y-1)'s left edge
        if (mby > 0) {
            uint32_t gv = 0;
            if (!gran_wait(gprev + (size_t)mbx * H264MI_DBK_GRANULES_PER_MB, 24, epoch, &gv, DD.abort_word)) return;
            if (lane < 16) *(uint32_t *)&S.L[(lane >> 2) * 20 + 4 + (lane & 3) * 4] = gv;
            else if (lane < 24) {
                const int pl = (lane - 16) >> 2, r = ((lane - 16) >> 1) & 1, hh = lane & 1;
                *(uint32_t *)&S.C[pl][r * 12 + 4 + hh * 4] = gv;
            }
        }
        wave_lds_sync();
        lap(2);
        const uint32_t sw = (uint32_t)__builtin_amdgcn_readlane((int)pf_i, 31);
        const int idc = MB_SLICE_IDC(sw), first = MB_SLICE_FIRST(sw), mbi = mby * mbw + mbx;
        const bool off = idc == 1;
        const int off_a = MB_SLICE_OFFA(sw), off_b = MB_SLICE_OFFB(sw);
        // idc 2: the left / top MB edge is not filtered when the MB across it is in another slice
        const bool lav = mbx > 0 && (idc != 2 || mbi - 1 >= first), tav = mby > 0 && (idc != 2 || mbi - mbw >= first);
        if (lane < 32) {  // one bs_of for every lane: the p-side MB and block indices are selected per lane
            const int dir = lane >> 4, e = (lane >> 2) & 3, s = lane & 3;
            const MbInfo &P = e != 0 ? S.cur : (dir == 0 ? S.left : S.top);
            const int rp = dir == 0 ? (e == 0 ? s * 4 + 3 : s * 4 + e - 1) : (e == 0 ? 12 + s : (e - 1) * 4 + s);
            const int rq = dir == 0 ? s * 4 + e : e * 4 + s;
            const bool avail = e != 0 || (dir == 0 ? lav : tav);
            const int b = bs_of(P, rp, S.cur, rq, e == 0);
            S.bs[dir][e][s] = (off || !avail) ? 0 : b;
        }
        // filter parameters of the three edge classes (left MB edge, top MB edge, internal), uniform
        // QPs from the record dwords in registers (lanes 0 / 1: this MB, 32 / 33: the MB above; the left
        // MB's carried over) rather than LDS reads -- qp_dbk / qpc_dbk on the packed fields
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)pf_i, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)pf_i, 1);
        const uint32_t a0 = (uint32_t)__builtin_amdgcn_readlane((int)pf_i, 32), a1 = (uint32_t)__builtin_amdgcn_readlane((int)pf_i, 33);
        const int qpq = (r0 & 255u) == MI_IPCM ? 0 : (int)((r0 >> 8) & 255u), qcq = (int)((r1 >> 8) & 255u);
        const int qpl = mbx > 0 ? left_qp : qpq, qcl = mbx > 0 ? left_qpc : qcq;
        const int qpt = mby > 0 ? ((a0 & 255u) == MI_IPCM ? 0 : (int)((a0 >> 8) & 255u)) : qpq, qct = mby > 0 ? (int)((a1 >> 8) & 255u) : qcq;
        left_qp = qpq; left_qpc = qcq;
        const EdgeQ LQ0 = edge_q((qpl + qpq + 1) >> 1, off_a, off_b), LQ1 = edge_q((qpt + qpq + 1) >> 1, off_a, off_b),
                    LQ2 = edge_q(qpq, off_a, off_b);
        const EdgeQ CQ0 = edge_q((qcl + qcq + 1) >> 1, off_a, off_b), CQ1 = edge_q((qct + qcq + 1) >> 1, off_a, off_b),
                    CQ2 = edge_q(qcq, off_a, off_b);
        wave_lds_sync();
        lap(3);
        // Lines in registers: lanes 0..15 luma (row or column `lane`), lanes 16..31 chroma (plane
        // (lane-16)>>3, line (lane-16)&7). v[0..19] = the line from -4 to 15 (chroma: -4..7; its
        // edges 0 and 4 take luma edge slots 0 and 1). Vertical edges first, then horizontal (8.7).
        if (lane < 32) {
            const bool ch = lane >= 16;
            const int pl = (lane - 16) >> 3, li = lane & 7;
            // every bS this lane's line meets, read before the passes (one LDS wait, not one per edge)
            int bsv[2][4];
#pragma unroll
            for (int dir = 0; dir < 2; dir++)
#pragma unroll
                for (int e = 0; e < 4; e++) bsv[dir][e] = !ch ? S.bs[dir][e][lane >> 2] : (e < 2 ? S.bs[dir][2 * e][li >> 1] : 0);
#pragma unroll
            for (int dir = 0; dir < 2; dir++) {
                int v[20];
                if (dir == 0) {
                    const uint32_t *row = ch ? (const uint32_t *)&S.C[pl][(li + 2) * 12] : (const uint32_t *)&S.L[(lane + 4) * 20];
#pragma unroll
                    for (int k = 0; k < 5; k++) {
                        const uint32_t w = (k < 3 || !ch) ? row[k] : 0u;
#pragma unroll
                        for (int j = 0; j < 4; j++) v[4 * k + j] = (w >> (8 * j)) & 255;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 20; k++) v[k] = ch ? (k >= 2 && k < 12 ? S.C[pl][(k - 2) * 12 + 4 + li] : 0) : S.L[k * 20 + 4 + lane];
                }
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int b = bsv[dir][e];
                    if (__ballot(b != 0) == 0) continue;  // no line of this edge is filtered (uniform)
                    const EdgeQ Ql = e == 0 ? (dir == 0 ? LQ0 : LQ1) : LQ2, Qc = e == 0 ? (dir == 0 ? CQ0 : CQ1) : CQ2;
                    const int alpha = ch ? Qc.alpha : Ql.alpha, beta = ch ? Qc.beta : Ql.beta;
                    const int t1 = ch ? Qc.t1 : Ql.t1, t2 = ch ? Qc.t2 : Ql.t2, t3 = ch ? Qc.t3 : Ql.t3;
                    if (e == 0) filt_reg<true>(v + 4 * e, b, alpha, beta, b == 1 ? t1 : (b == 2 ? t2 : t3), ch);
                    else filt_reg<false>(v + 4 * e, b, alpha, beta, b == 1 ? t1 : (b == 2 ? t2 : t3), ch);  // internal: bS <= 3
                }
                if (dir == 0) {
                    uint32_t *row = ch ? (uint32_t *)&S.C[pl][(li + 2) * 12] : (uint32_t *)&S.L[(lane + 4) * 20];
#pragma unroll
                    for (int k = 0; k < 5; k++)
                        if (k < 3 || !ch) row[k] = (uint32_t)v[4 * k] | ((uint32_t)v[4 * k + 1] << 8) | ((uint32_t)v[4 * k + 2] << 16) | ((uint32_t)v[4 * k + 3] << 24);
                } else {
#pragma unroll
                    for (int k = 1; k < 20; k++) {  // row -4 (p3 of the top edge) is never written
                        if (!ch) S.L[k * 20 + 4 + lane] = (uint8_t)v[k];
                        else if (k >= 2 && k < 12) S.C[pl][(k - 2) * 12 + 4 + li] = (uint8_t)v[k];
                    }
                }
                wave_lds_sync();
            }
        }
        wave_lds_sync();
        lap(4);
        // ---- rows 13..15 (chroma row 7) of the MB above are final now
        if (mby > 0) {
            if (lane < 12) {
                const int r = 1 + (lane >> 2), c4 = (lane & 3) * 4;
                *(GLOBAL uint32_t *)&D.dbk[0][(size_t)(Y - 4 + r) * cw + X + c4] = *(const uint32_t *)&S.L[r * 20 + 4 + c4];
            } else if (lane >= 16 && lane < 20) {
                const int pl = (lane - 16) >> 1, hh = lane & 1;
                *(GLOBAL uint32_t *)&D.chroma(pl)[(size_t)(mby * 8 - 1) * ccw + mbx * 8 + hh * 4] = *(const uint32_t *)&S.C[pl][1 * 12 + 4 + hh * 4];
            }
        }
        // ---- MB x-1 is complete for this row: update its right columns and flush it
        if (mbx > 0) {
            { int r = lane >> 2, c = lane & 3; S.prev[r * 16 + 12 + c] = S.L[(r + 4) * 20 + c]; }
            if (lane < 32) { int pl = lane >> 4, r = (lane >> 1) & 7, c = lane & 1; S.prevc[pl][r * 8 + 6 + c] = S.C[pl][(r + 2) * 12 + 2 + c]; }
            wave_lds_sync();
            dbk_flush(S, D, grow, epoch, mbx - 1, mby, cw, last_row);
        }
        wave_lds_sync();
        *(uint32_t *)&S.prev[lane * 4] = *(const uint32_t *)&S.L[((lane >> 2) + 4) * 20 + 4 + (lane & 3) * 4];
        if (lane < 32) {
            const int pl = lane >> 4, r = (lane >> 1) & 7, hh = lane & 1;
            *(uint32_t *)&S.prevc[pl][r * 8 + hh * 4] = *(const uint32_t *)&S.C[pl][(r + 2) * 12 + 4 + hh * 4];
            ((uint32_t *)&S.left)[lane] = ((const uint32_t *)&S.cur)[lane];
        }
        wave_lds_sync();
        if (mbx == mbw - 1) dbk_flush(S, D, grow, epoch, mbx, mby, cw, last_row);
        lap(5);
    }
    if (a.prof && lane == 0)
#pragma unroll
        for (int k = 1; k < 6; k++) atomicAdd((unsigned long long *)&a.prof[k], (unsigned long long)s_prof[k]);
}

__global__ __launch_bounds__(64) void deblock_kernel(DbkLaunch a) {
    __shared__ DbkLds S;
    __shared__ int s_ticket;
    if (threadIdx.x == 0) s_ticket = (int)atomicAdd(a.ticket, 1u);
    wave_lds_sync();
    const int t = uni(s_ticket), mby = t / a.S, sidx = t % a.S;
    if (mby >= a.mbh) return;
    CONSTANT const DbkDesc &DD = cst(a.desc)[sidx];
    DbkSrcGlobal src{gbl(DD.rec[0]), gbl(DD.rec[1]), gbl(DD.rec[2]), gbl((const uint32_t *)DD.info), a.mbw * 16, a.mbw, mby};
    deblock_row(S, a, DD, mby, src);
}

}  // namespace h264mi
