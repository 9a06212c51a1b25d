// dec_recon.inc -- decoder reconstruction (gfx950): intra prediction (8.3), inter prediction
// with luma 6-tap quarter-sample / chroma eighth-sample interpolation (8.4.2.2), inverse transform
// + dequantisation (8.5), from the per-MB records of dec_parse.inc.
//
// Replaces the reconstruction half of ISVCDecoder::DecodeFrameNoDelay (openh264_wrapper.cpp:435).
// The parse is finished here too: motion vectors (8.4.1) and Intra4x4 modes (8.3.1.1) are resolved from the
// raw record by one set of rule functions (rnb .. resolve_record), run in one of two places. A call whose
// slice data is parsed before its reconstruction starts resolves every picture's records in dec_resolve_kernel,
// a light row wavefront ahead of the reconstruction, and dec_recon_kernel<true> reads resolved records: its
// inter macroblocks wait for nothing from their own picture. A streamed call (the reconstruction follows the
// slice data row by row) keeps the resolution inside the reconstruction wavefront, dec_recon_kernel<false>,
// with the above row's bottom vectors/modes arriving as granules 8..12.
// Same MB-row wavefront as the encoder: one wave per (stream, MB row); the unfiltered bottom line
// of each MB is handed to the row below as {epoch,payload} granules. Residuals of all 24 blocks
// are computed in parallel (lane per block); the only serial chain is the Intra4x4 one (16 steps of
// 16-lane prediction+add).
// Inter prediction reads one reference plane: the edge-padded integer picture G (dec_planes_kernel,
// enc_planes.inc), of which each row wave keeps columns [X-24, X+40) of rows [Y-24, Y+40) in a 64-column
// LDS ring (the encoder's window geometry, one plane instead of its four). A decoder samples every block
// once, at a vector it knows, so the half-sample values b, h, j are computed where they are used
// (8.4.2.2.1, six-tap filters over the window, in registers) and are never stored. A macroblock whose
// vectors are all whole-sample reads its four samples per lane and nothing else. A macroblock with a
// block whose filter footprint leaves the window (mb_in_window) interpolates from the deblocked picture
// in HBM with clamping (GlobGet).
namespace h264mi {

// prof: 16 section totals (diagnostic); streamed: the slice data is still being parsed -- each row waits
// for its records (DecFrame::prog, tag = the call's)
struct DecLaunch { int S, mbw, mbh; const DecDesc *desc; uint32_t *ticket; const DbkDesc *dbk; uint64_t *prof; uint32_t tag; int streamed; };

// Streamed reconstruction gate (one wave, ahead of dec_recon_kernel on its stream): returns once every
// stream's slice data of the frame has published `rows` MB rows (or finished, or failed). The reconstruction
// launch queued behind it then follows only the tail of the parse, so its waiting waves do not hold the CUs
// for the whole of a long slice (other kernels -- an encoder's -- need them meanwhile). Bounded polls.
struct DecGateLaunch { int S; const DecDesc *desc; uint32_t tag; uint32_t rows; };
__global__ __launch_bounds__(64) void dec_gate_kernel(DecGateLaunch a) {
    for (int s = 0; s < a.S; s++) {
        const DecDesc &D = a.desc[s];
        if (!D.st->got_pic) continue;
        GLOBAL uint64_t *prog = gbl(&D.frm->prog);
        WaitClock wc;  // bounded like every wait (the gate is a scheduling hint: the launch behind it is correct anyway)
        for (unsigned spins = 0; ((spins & 255) != 255) || !wc.expired(); spins++) {
            uint64_t x = 0;
            if (threadIdx.x == 0) x = __hip_atomic_load(prog, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32));
            const uint32_t v = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
            if (t == a.tag && v >= a.rows) break;  // (the abort value is >= any row count)
            __builtin_amdgcn_s_sleep(8);
        }
    }
}

// Reconstruction gate (h264mi_dec_set_recon_gate): one wave holds the reconstruction stream until a device
// counter another kernel advances (an encoder's rows-started counter) reaches `target` (wrap-safe), or until
// `limit_ticks` of the 100 MHz clock have passed -- a scheduling hint only: the launch behind it is correct
// whenever it runs. Lets a caller start each frame's reconstruction in the tail of a concurrent encoder launch,
// when most of the encoder's rows have retired, instead of beside its densest part.
struct DecWaitLaunch { const uint32_t *counter; uint32_t target; uint32_t limit_ticks; };
__global__ __launch_bounds__(64) void dec_wait_counter_kernel(DecWaitLaunch a) {
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        uint32_t x = 0;
        if (threadIdx.x == 0) x = __hip_atomic_load(a.counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
        if ((int32_t)(x - a.target) >= 0) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > a.limit_ticks) break;
        __builtin_amdgcn_s_sleep(8);
    }
}

// Streamed reconstruction: wait until the slice-data waves have published MB row `need` - 1 (the rows'
// records and coefficients are in memory), then acquire. An abort (the slice data failed) stops the
// frame's wavefront through its abort word. Bounded like gran_wait.
DEV bool prog_wait(GLOBAL uint64_t *prog, uint32_t tag, uint32_t need, int32_t *abort_word) {
    WaitClock wc;
    for (unsigned spins = 0;; spins++) {
        uint64_t x = 0;
        if (threadIdx.x == 0) x = __hip_atomic_load(prog, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32));
        const uint32_t v = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
        if (t == tag) {
            if (v == H264MI_PROG_ABORT) break;
            if (v >= need) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                return true;
            }
        }
        if ((spins & 255) == 255) {
            const int ab = __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ab || wc.expired()) break;
        }
        __builtin_amdgcn_s_sleep(2);
    }
    if (threadIdx.x == 0) __hip_atomic_store(abort_word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return false;
}

// MBs whose vectors leave the window interpolate from the deblocked picture in HBM and I_PCM samples are read
// from the coefficient image (an LDS tile for the former and an LDS copy of the latter cost a workgroup per CU
// and 1.4 % of the bench when the windows held four planes, profiles/round5/ab_recon_notile.txt).
constexpr int DWIN_ROWS = 64;            // window rows [Y-24, Y+40), one per lane of the strip loads
constexpr int DWIN_LO = -24, DWIN_HI = 40;   // luma window, rows and columns relative to the MB: [DWIN_LO, DWIN_HI)
constexpr int DWINC_LO = -12, DWINC_HI = 20; // chroma window
struct DecLds {
    alignas(16) uint8_t win[DWIN_ROWS * WIN_RING];  // integer reference plane G: 64-column ring (enc_mb.inc layout)
    alignas(16) uint8_t winc[2][32 * 32];  // Cb, Cr ring
    alignas(16) uint32_t cf[208];          // this MB's MbCoef image (only blocks with TotalCoeff > 0 are valid)
    alignas(16) int16_t res[24][16];
    int dcval[24];                      // reconstructed DC coefficients (I16 luma 0..15, chroma 16..23)
    alignas(16) uint8_t rec[256];
    alignas(16) uint8_t recc[2][64];
    uint8_t top[24];
    uint8_t topc[2][12];
    uint8_t left[16], leftc[2][8];
    uint8_t n4[16];
    uint32_t gp[3][8];
    uint32_t gm[3][5];   // above-row MBs: bottom-row mvs (ras 12..15), type | bottom Intra4x4 modes << 8
    int8_t modes[16];
    alignas(16) MbInfo info;
    alignas(16) MbInfo linfo;  // resolved record of the left MB
};

// 4 window bytes at absolute column gx of window row wr (ring of 64 columns, enc_mb.inc layout)
DEV uint32_t dwin4(const DecLds &S, int wr, int gx) {
    const int sl = (gx + 24) & 63;
    const uint32_t *row = (const uint32_t *)&S.win[wr * WIN_RING];
    return __builtin_amdgcn_alignbyte(row[((sl >> 2) + 1) & 15], row[sl >> 2], sl & 3);
}

// ---------------------------------------------------------------- luma interpolation from the G window
// Samples gx-2 .. gx+6 of window row wr, the footprint of the horizontal six-tap filter over a lane's four
// samples gx..gx+3: lo = samples 0..3 of the nine, mid = 4..7, hi = the ninth. Three ring dwords whatever
// the alignment. The row index is clamped to the window: mb_in_window admits a macroblock only if every row
// a lane *uses* is inside, and a lane that computes a filter for its neighbours' sake (the filters run under
// wave-uniform branches) then reads some valid row and drops the result.
struct WRow { uint32_t lo, mid, hi; };
DEV WRow dwin_row(const DecLds &S, int wr, int gx) {
    const int sl = (gx - 2 + 24) & 63, d = sl >> 2, sh = sl & 3;
    const uint32_t *row = (const uint32_t *)&S.win[clip3(0, DWIN_ROWS - 1, wr) * WIN_RING];
    const uint32_t d0 = row[d], d1 = row[(d + 1) & 15], d2 = row[(d + 2) & 15];
    return WRow{__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh), (d2 >> (8 * sh)) & 255u};
}
// the lane's four samples of the row, at column offset dx (0 or 1)
DEV uint32_t wrow_quad(const WRow &r, int dx) { return __builtin_amdgcn_alignbyte(r.mid, r.lo, 2 + dx); }
// unrounded horizontal taps b1 (8-241) of the lane's four samples
DEV void wrow_b1(const WRow &r, int t[4]) {
    int s[9];
#pragma unroll
    for (int k = 0; k < 4; k++) { s[k] = (r.lo >> (8 * k)) & 255; s[4 + k] = (r.mid >> (8 * k)) & 255; }
    s[8] = r.hi;
#pragma unroll
    for (int k = 0; k < 4; k++) t[k] = tap6(s[k], s[k + 1], s[k + 2], s[k + 3], s[k + 4], s[k + 5]);
}
DEV uint32_t pack_clip_shr(const int t[4], int rnd, int sh) {
    uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) o |= (uint32_t)clip1_shr(t[k] + rnd, sh) << (8 * k);
    return o;
}
// 8.4.2.2.1 for a macroblock with at least one fractional vector: four prediction samples per lane (columns
// gx..gx+3 of window row wr, position idx = yFrac * 4 + xFrac of the lane's 4x4 block). Every position is the
// rounded average of two of {G, b, h, j} at the offsets qsel() tabulates (at most one operand of each kind),
// with b = Clip1((b1 + 16) >> 5), h likewise down the column, j = Clip1((tap6 of six rows' b1 + 512) >> 10)
// -- the formulas the encoder's planes hold (enc_planes.inc), over the same edge-padded G. The blocks of one
// macroblock may differ in position: which of the three filters any lane needs is decided for the wave with a
// ballot, every lane runs those and selects its operands; no per-lane branch. Whole wave: every lane active.
DEV uint32_t dec_luma_frac(const DecLds &S, int wr, int gx, int idx) {
    const QSel q = qsel(idx);
    const bool ub = __ballot(q.p1 == 1 || q.p2 == 1) != 0, uh = __ballot(q.p1 == 2 || q.p2 == 2) != 0;
    const bool uj = __ballot(q.p1 == 3 || q.p2 == 3) != 0;
    const int gdx = q.p1 == 0 ? q.dx1 : q.dx2, gdy = q.p1 == 0 ? q.dy1 : q.dy2;  // the G operand's offset
    const int bdy = q.p1 == 1 ? q.dy1 : q.dy2, hdx = q.p1 == 2 ? q.dx1 : q.dx2;  // b's row, h's column offset
    const WRow r2 = dwin_row(S, wr, gx);
    WRow r3 = r2;  // row wr + 1: only positions with yFrac 3 read it, and those need h or j
    uint32_t vb = 0, vh = 0, vj = 0;
    if (uh || uj) {
        const WRow r0 = dwin_row(S, wr - 2, gx), r1 = dwin_row(S, wr - 1, gx), r4 = dwin_row(S, wr + 2, gx), r5 = dwin_row(S, wr + 3, gx);
        r3 = dwin_row(S, wr + 1, gx);
        if (uh) {
            const uint32_t c0 = wrow_quad(r0, hdx), c1 = wrow_quad(r1, hdx), c2 = wrow_quad(r2, hdx), c3 = wrow_quad(r3, hdx);
            const uint32_t c4 = wrow_quad(r4, hdx), c5 = wrow_quad(r5, hdx);
            int t[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int s = 8 * k;
                t[k] = tap6((c0 >> s) & 255, (c1 >> s) & 255, (c2 >> s) & 255, (c3 >> s) & 255, (c4 >> s) & 255, (c5 >> s) & 255);
            }
            vh = pack_clip_shr(t, 16, 5);
        }
        if (uj) {
            int t0[4], t1[4], t2[4], t3[4], t4[4], t5[4], t[4];
            wrow_b1(r0, t0); wrow_b1(r1, t1); wrow_b1(r2, t2); wrow_b1(r3, t3); wrow_b1(r4, t4); wrow_b1(r5, t5);
#pragma unroll
            for (int k = 0; k < 4; k++) t[k] = tap6(t0[k], t1[k], t2[k], t3[k], t4[k], t5[k]);
            vj = pack_clip_shr(t, 512, 10);
        }
    }
    if (ub) {
        const WRow rb{bdy ? r3.lo : r2.lo, bdy ? r3.mid : r2.mid, bdy ? r3.hi : r2.hi};
        int t[4];
        wrow_b1(rb, t);
        vb = pack_clip_shr(t, 16, 5);
    }
    const uint32_t vg = gdy ? wrow_quad(r3, 0) : wrow_quad(r2, gdx);
    const uint32_t pa = q.p1 == 0 ? vg : (q.p1 == 1 ? vb : (q.p1 == 2 ? vh : vj));
    const uint32_t pb = q.p2 == 0 ? vg : (q.p2 == 1 ? vb : (q.p2 == 2 ? vh : vj));
    return (pa | pb) - (((pa ^ pb) & 0xFEFEFEFEu) >> 1);  // bytewise (a + b + 1) >> 1
}

struct GlobGet {
    GLOBAL const uint8_t *p; int w, h;
    DEV int operator()(int x, int y) const { return p[clip3(0, h - 1, y) * w + clip3(0, w - 1, x)]; }
};
template <class G> DEV int g_b1(const G &g, int x, int y) { return tap6(g(x - 2, y), g(x - 1, y), g(x, y), g(x + 1, y), g(x + 2, y), g(x + 3, y)); }
template <class G> DEV int g_b(const G &g, int x, int y) { return clip1((g_b1(g, x, y) + 16) >> 5); }
template <class G> DEV int g_h(const G &g, int x, int y) {
    return clip1((tap6(g(x, y - 2), g(x, y - 1), g(x, y), g(x, y + 1), g(x, y + 2), g(x, y + 3)) + 16) >> 5);
}
template <class G> DEV int g_j(const G &g, int x, int y) {
    return clip1((tap6(g_b1(g, x, y - 2), g_b1(g, x, y - 1), g_b1(g, x, y), g_b1(g, x, y + 1), g_b1(g, x, y + 2), g_b1(g, x, y + 3)) + 512) >> 10);
}
// 8.4.2.2.1 luma sample (same table as the encoder's window sampler)
template <class G> DEV int qpel(const G &g, int x, int y, int fx, int fy) {
    switch (fy * 4 + fx) {
    case 0: return g(x, y);
    case 1: return AVG(g(x, y), g_b(g, x, y));
    case 2: return g_b(g, x, y);
    case 3: return AVG(g_b(g, x, y), g(x + 1, y));
    case 4: return AVG(g(x, y), g_h(g, x, y));
    case 5: return AVG(g_b(g, x, y), g_h(g, x, y));
    case 6: return AVG(g_b(g, x, y), g_j(g, x, y));
    case 7: return AVG(g_b(g, x, y), g_h(g, x + 1, y));
    case 8: return g_h(g, x, y);
    case 9: return AVG(g_h(g, x, y), g_j(g, x, y));
    case 10: return g_j(g, x, y);
    case 11: return AVG(g_j(g, x, y), g_h(g, x + 1, y));
    case 12: return AVG(g_h(g, x, y), g(x, y + 1));
    case 13: return AVG(g_h(g, x, y), g_b(g, x, y + 1));
    case 14: return AVG(g_j(g, x, y), g_b(g, x, y + 1));
    default: return AVG(g_h(g, x + 1, y), g_b(g, x, y + 1));
    }
}

// ---------------------------------------------------------------- record resolution (lane 0)
// The parse kernel leaves mvd and raw Intra4x4 mode codes in the record; the wavefront resolves
// them here because every prediction input is a neighbour it already holds: the left MB's resolved
// record (S.linfo) and, from the row above, granules 8..12 of MBs x-1, x, x+1 (S.gm).
struct RNb { int avail, ref, mx, my; };
// neighbour MB availability of the current MB (6.4.8: inside the picture and in the same slice), bits:
// 1 left (A), 2 top (B), 4 top-right (C), 8 top-left (D)
enum { NB_A = 1, NB_B = 2, NB_C = 4, NB_D = 8 };
DEV uint32_t mb_nb_mask(int mbx, int mby, int mbw, int first) {
    const int mbi = mby * mbw + mbx;
    return (mbx > 0 && mbi - 1 >= first ? NB_A : 0) | (mby > 0 && mbi - mbw >= first ? NB_B : 0) |
           (mby > 0 && mbx + 1 < mbw && mbi - mbw + 1 >= first ? NB_C : 0) | (mby > 0 && mbx > 0 && mbi - mbw - 1 >= first ? NB_D : 0);
}
template <class L> DEV RNb rnb(const L &S, int mbx, uint32_t nbm, uint32_t done, int x, int y) {
    RNb r = {0, -1, 0, 0};
    if (y < 0) {
        const uint32_t *g;
        int nx;
        if (x < 0) { if (!(nbm & NB_D)) return r; g = S.gm[(mbx + 2) % 3]; nx = x + 16; }
        else if (x < 16) { if (!(nbm & NB_B)) return r; g = S.gm[mbx % 3]; nx = x; }
        else { if (!(nbm & NB_C)) return r; g = S.gm[(mbx + 1) % 3]; nx = x - 16; }
        r.avail = 1;
        const int t = g[4] & 255;
        if (t == MI_I4 || t == MI_I16 || t == MI_IPCM) return r;
        const uint32_t mv = g[nx >> 2];
        r.ref = 0; r.mx = (int16_t)(mv & 0xffff); r.my = (int16_t)(mv >> 16);
        return r;
    }
    if (x < 0) {
        if (!(nbm & NB_A)) return r;
        r.avail = 1;
        const int t = S.linfo.type;
        if (t == MI_I4 || t == MI_I16 || t == MI_IPCM) return r;
        const int ras = (y >> 2) * 4 + 3;
        r.ref = 0; r.mx = S.linfo.mv[ras][0]; r.my = S.linfo.mv[ras][1];
        return r;
    }
    if (x >= 16) return r;
    const int ras = (y >> 2) * 4 + (x >> 2);
    if (!((done >> ras) & 1)) return r;
    r.avail = 1; r.ref = 0; r.mx = S.info.mv[ras][0]; r.my = S.info.mv[ras][1];
    return r;
}
// 8.4.1.3 (shape 0: median, 1: 16x8, 2: 8x16)
template <class L> DEV void rmvp(const L &S, int mbx, uint32_t nbm, uint32_t done, int bx, int by, int pw, int shape, int &ox, int &oy) {
    RNb A = rnb(S, mbx, nbm, done, bx - 1, by), B = rnb(S, mbx, nbm, done, bx, by - 1);
    RNb C = rnb(S, mbx, nbm, done, bx + pw, by - 1);
    if (!C.avail) C = rnb(S, mbx, nbm, done, bx - 1, by - 1);
    if (shape == 1) {
        if (by == 0 && B.ref == 0) { ox = B.mx; oy = B.my; return; }
        if (by != 0 && A.ref == 0) { ox = A.mx; oy = A.my; return; }
    } else if (shape == 2) {
        if (bx == 0 && A.ref == 0) { ox = A.mx; oy = A.my; return; }
        if (bx != 0 && C.ref == 0) { ox = C.mx; oy = C.my; return; }
    }
    if (!B.avail && !C.avail && A.avail) { B = A; C = A; }
    const int n = (A.ref == 0) + (B.ref == 0) + (C.ref == 0);
    if (n == 1) {
        const RNb &q = A.ref == 0 ? A : (B.ref == 0 ? B : C);
        ox = q.mx; oy = q.my;
        return;
    }
    ox = median3(A.mx, B.mx, C.mx);
    oy = median3(A.my, B.my, C.my);
}
DEV void set_part_mv(MbInfo &I, uint32_t &done, int px, int py, int pw, int ph, int mx, int my) {
    for (int y = py; y < py + ph; y += 4)
        for (int x = px; x < px + pw; x += 4) {
            const int ras = (y >> 2) * 4 + (x >> 2);
            I.mv[ras][0] = (int16_t)mx; I.mv[ras][1] = (int16_t)my;
            done |= 1u << ras;
        }
}
// P_Skip and P_L0_16x16 (most macroblocks of a P picture), wave-uniform: the neighbour words are read
// into scalars (8.4.1.1 / 8.4.1.3, the same decisions as rnb / rmvp for a 16x16 partition) and the 16
// block vectors are written by 16 lanes at once instead of one lane's loop.
template <class L> DEV uint32_t resolve_p16_uni(L &S, int mbx, uint32_t nbm, bool skip) {
    // every neighbour word first (one LDS round trip instead of one per neighbour behind its branch)
    const int sb = mbx % 3, sc = sb == 2 ? 0 : sb + 1, sd = sb == 0 ? 2 : sb - 1;
    const uint32_t wa_t = S.linfo.type, wa_mv = ((const uint32_t *)S.linfo.mv)[3];
    const uint32_t wb_t = S.gm[sb][4], wb_mv = S.gm[sb][0], wc_t = S.gm[sc][4], wc_mv = S.gm[sc][0];
    const uint32_t wd_t = S.gm[sd][4], wd_mv = S.gm[sd][3], wmvd = ((const uint32_t *)S.info.mv)[0];
    auto nb = [](bool avail, uint32_t t, uint32_t mv) {
        RNb r = {0, -1, 0, 0};
        if (!avail) return r;
        r.avail = 1;
        t = uni(t) & 255;
        if (t == MI_I4 || t == MI_I16 || t == MI_IPCM) return r;
        mv = uni(mv);
        r.ref = 0; r.mx = (int16_t)(mv & 0xffff); r.my = (int16_t)(mv >> 16);
        return r;
    };
    RNb A = nb(nbm & NB_A, wa_t, wa_mv), B = nb(nbm & NB_B, wb_t, wb_mv);
    int mx = 0, my = 0;
    const bool zero_skip = skip && ((nbm & (NB_A | NB_B)) != (NB_A | NB_B) || (A.ref == 0 && A.mx == 0 && A.my == 0) ||
                                    (B.ref == 0 && B.mx == 0 && B.my == 0));
    if (!zero_skip) {
        RNb C = nb(nbm & NB_C, wc_t, wc_mv);
        if (!C.avail) C = nb(nbm & NB_D, wd_t, wd_mv);
        if (!B.avail && !C.avail && A.avail) { B = A; C = A; }
        const int n = (A.ref == 0) + (B.ref == 0) + (C.ref == 0);
        if (n == 1) {
            const RNb &q = A.ref == 0 ? A : (B.ref == 0 ? B : C);
            mx = q.mx; my = q.my;
        } else {
            mx = median3(A.mx, B.mx, C.mx);
            my = median3(A.my, B.my, C.my);
        }
    }
    if (!skip) {  // + the mvd the parse left at block 0
        const uint32_t d = uni(wmvd);
        mx += (int16_t)(d & 0xffff); my += (int16_t)(d >> 16);
    }
    const int lane = threadIdx.x & 63;
    const uint32_t mvw = (uint32_t)(uint16_t)mx | ((uint32_t)(uint16_t)my << 16);
    if (lane < 16) ((uint32_t *)S.info.mv)[lane] = mvw;
    return mvw;  // every block's vector (uniform)
}
template <class L> DEV void resolve_record(L &S, int mbx, uint32_t nbm) {
    MbInfo &I = S.info;
    const int type = I.type;
    uint32_t done = 0;
    if (type == MI_PSKIP) {  // 8.4.1.1
        int mx = 0, my = 0;
        if ((nbm & (NB_A | NB_B)) == (NB_A | NB_B)) {
            RNb A = rnb(S, mbx, nbm, 0, -1, 0), B = rnb(S, mbx, nbm, 0, 0, -1);
            if (!(A.ref == 0 && A.mx == 0 && A.my == 0) && !(B.ref == 0 && B.mx == 0 && B.my == 0))
                rmvp(S, mbx, nbm, 0, 0, 0, 16, 0, mx, my);
        }
        set_part_mv(I, done, 0, 0, 16, 16, mx, my);
    } else if (type == MI_P16x16 || type == MI_P16x8 || type == MI_P8x16) {
        const int n = type == MI_P16x16 ? 1 : 2, shape = type == MI_P16x16 ? 0 : (type == MI_P16x8 ? 1 : 2);
        for (int i = 0; i < n; i++) {
            const int px = shape == 2 ? 8 * i : 0, py = shape == 1 ? 8 * i : 0;
            const int pw = shape == 2 ? 8 : 16, ph = shape == 1 ? 8 : 16;
            const int ras = (py >> 2) * 4 + (px >> 2);
            const int dx = I.mv[ras][0], dy = I.mv[ras][1];
            int mx, my;
            rmvp(S, mbx, nbm, done, px, py, pw, shape, mx, my);
            set_part_mv(I, done, px, py, pw, ph, mx + dx, my + dy);
        }
    } else if (type == MI_P8x8) {
        for (int i = 0; i < 4; i++) {
            const int sb = I.sub[i];
            const int sw = (sb == 0 || sb == 1) ? 8 : 4, sh = (sb == 0 || sb == 2) ? 8 : 4;
            for (int y = 0; y < 8; y += sh)
                for (int x = 0; x < 8; x += sw) {
                    const int px = (i & 1) * 8 + x, py = (i >> 1) * 8 + y;
                    const int ras = (py >> 2) * 4 + (px >> 2);
                    const int dx = I.mv[ras][0], dy = I.mv[ras][1];
                    int mx, my;
                    rmvp(S, mbx, nbm, done, px, py, sw, 0, mx, my);
                    set_part_mv(I, done, px, py, sw, sh, mx + dx, my + dy);
                }
        }
    } else if (type == MI_I4) {  // 8.3.1.1
        for (int blk = 0; blk < 16; blk++) S.modes[blk] = I.i4mode[blk];
        const uint32_t top = S.gm[mbx % 3][4] >> 8;
        for (int blk = 0; blk < 16; blk++) {
            const int ras = BLK2RAS[blk], x4 = ras & 3, y4 = ras >> 2;
            const int ma = x4 > 0 ? I.i4mode[ras - 1] : ((nbm & NB_A) ? S.linfo.i4mode[ras + 3] : -1);
            const int mb = y4 > 0 ? I.i4mode[ras - 4] : ((nbm & NB_B) ? (int)((top >> (4 * x4)) & 15) : -1);
            const int pm = (ma < 0 || mb < 0) ? 2 : min(ma, mb);
            const int code = (uint8_t)S.modes[blk];
            I.i4mode[ras] = (int8_t)(code == 0xff ? pm : (code < pm ? code : code + 1));
        }
    }
}

// what the row below needs of a resolved record besides its bottom vectors: type | bottom Intra4x4 modes << 8
DEV uint32_t res_type_word(const MbInfo &R) {
    return (uint32_t)R.type | ((uint32_t)(R.i4mode[12] & 15) << 8) | ((uint32_t)(R.i4mode[13] & 15) << 12) |
           ((uint32_t)(R.i4mode[14] & 15) << 16) | ((uint32_t)(R.i4mode[15] & 15) << 20);
}

// ---------------------------------------------------------------- resolution pass
// dec_resolve_kernel: the raw records of every picture of a call -> resolved records (mv[16], i4mode[16]), in
// place, before any of the call's pictures is reconstructed. None of it depends on samples, and in Baseline on
// no other picture, so all `np` pictures (frames x streams) resolve at once: one wave per (picture, MB row), in
// ticket order rows-major, so a row waits only for lower tickets (the forward-progress argument of the other
// wavefront kernels). Row y hands the vectors of its bottom blocks, its type and its bottom Intra4x4 modes to
// row y + 1 as 5 {tag, payload} granules per MB (DecDesc::rgran, per frame slot; the tag is the call's, so a
// slot's granules of an earlier call are stale), and keeps MBs x-1, x, x+1 of the row above in the three-slot
// gm ring the rule functions read. Waits are gran_wait's: bounded by WaitClock, ended by the picture's abort
// word (DecFrame::res_abort; dec_frame_begin_kernel then drops the picture). No samples, coefficients or
// reference windows: 5 KB less LDS and a fifth of the reconstruction's registers.
#define H264MI_RES_GRANULES_PER_MB 5
struct DecResolveLaunch { int np, mbw, mbh; const DecDesc *desc; uint32_t *ticket; uint32_t base, tag; int conceal; };
struct ResLds {
    uint32_t gm[3][5];         // above-row MBs, as DecLds::gm
    int8_t modes[16];
    alignas(16) MbInfo info;
    alignas(16) MbInfo linfo;  // resolved record of the left MB
};
__global__ __launch_bounds__(64) void dec_resolve_kernel(DecResolveLaunch a) {
    __shared__ ResLds S;
    __shared__ int s_ticket;
    const int lane = threadIdx.x;
    // the counter is never reset: the host passes the value it had before this launch (launches that share a
    // counter are ordered on one stream or by the slot group's events)
    if (lane == 0) s_ticket = (int)(atomicAdd(a.ticket, 1u) - a.base);
    wave_lds_sync();
    const int t = uni(s_ticket);
    if (t < 0 || t >= a.np * a.mbh) return;
    const int mby = t / a.np, w = t - mby * a.np;
    CONSTANT const DecDesc &D = cst(a.desc)[w];
    DecFrame *F = D.frm;
    // the pictures dec_frame_begin_kernel may accept (it also wants a reference for P slices, which only the
    // reconstruction side knows: a picture resolved for nothing costs nothing else)
    // (with concealment on, also the pictures whose gaps dec_conceal_kernel filled)
    if (!uni(F->hdr_ok) || uni(F->err) || !uni((int)(slices_cover(F) || (a.conceal && F->ncon > 0)))) return;
    int32_t *abort_word = &F->res_abort;
    const uint32_t tag = a.tag;
    const int mbw = a.mbw;
    GLOBAL uint32_t *info32 = gbl((uint32_t *)D.info) + (size_t)mby * mbw * 32;
    GLOBAL uint64_t *grow = gbl(D.rgran) + (size_t)mby * mbw * H264MI_RES_GRANULES_PER_MB;
    GLOBAL uint64_t *grow_prev = grow - (mby > 0 ? (size_t)mbw * H264MI_RES_GRANULES_PER_MB : 0);
    const bool below = mby + 1 < a.mbh;
    // one MB ahead: the raw record, and the row above's granules of MB x+2 (polled again only if still stale)
    uint32_t pf_info = lane < 32 ? info32[lane] : 0;
    uint64_t pf_g = 0;
    auto gload = [&](int mx) {
        if (lane < 5) pf_g = __hip_atomic_load(grow_prev + (size_t)mx * H264MI_RES_GRANULES_PER_MB + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto gtake = [&](int mx) -> bool {  // MB mx of the row above -> its gm slot
        uint32_t v = (uint32_t)pf_g;
        if (__ballot(lane < 5 && (uint32_t)(pf_g >> 32) != tag) != 0 &&
            !gran_wait(grow_prev + (size_t)mx * H264MI_RES_GRANULES_PER_MB, 5, tag, &v, abort_word)) return false;
        if (lane < 5) S.gm[mx % 3][lane] = v;
        return true;
    };
    if (mby > 0) {
        gload(0);
        if (!gtake(0)) return;
        if (mbw > 1) gload(1);
    }
    for (int mbx = 0; mbx < mbw; mbx++) {
        if (lane < 32) ((uint32_t *)&S.info)[lane] = pf_info;
        const uint32_t rw0 = __builtin_amdgcn_readfirstlane(pf_info), rw31 = __builtin_amdgcn_readlane(pf_info, 31);
        const int rt = (int)(rw0 & 255);
        if (mbx + 1 < mbw && lane < 32) pf_info = info32[(size_t)(mbx + 1) * 32 + lane];
        if (mby > 0 && mbx + 1 < mbw) {
            if (!gtake(mbx + 1)) return;
            if (mbx + 2 < mbw) gload(mbx + 2);
        }
        wave_lds_sync();
        const uint32_t nbm = uni(mb_nb_mask(mbx, mby, mbw, MB_SLICE_FIRST(rw31)));
        if (rt == MI_PSKIP || rt == MI_P16x16) resolve_p16_uni(S, mbx, nbm, rt == MI_PSKIP);
        else if (lane == 0) resolve_record(S, mbx, nbm);
        wave_lds_sync();
        const uint32_t rv = lane < 32 ? ((const uint32_t *)&S.info)[lane] : 0;
        if (below && lane < 5) gran_store(grow + (size_t)mbx * H264MI_RES_GRANULES_PER_MB + lane, tag, lane < 4 ? ((const uint32_t *)S.info.mv)[12 + lane] : res_type_word(S.info));
        // the resolved fields back into the record: i4mode (dwords 2..5) and mv (15..30)
        static_assert(offsetof(MbInfo, i4mode) == 8 && offsetof(MbInfo, mv) == 60, "MbInfo dwords of the resolved fields");
        if ((lane >= 2 && lane < 6) || (lane >= 15 && lane < 31)) info32[(size_t)mbx * 32 + lane] = rv;
        if (lane < 32) ((uint32_t *)&S.linfo)[lane] = rv;
        wave_lds_sync();
    }
}

// Every sample the window paths read for the MB's 4x4 blocks lies inside the LDS windows: luma columns/rows
// [DWIN_LO, DWIN_HI) = [-24, 40) and chroma [DWINC_LO, DWINC_HI) = [-12, 20) relative to the MB. Exact, per
// block and per direction:
//   luma    the block's samples p .. p+3 at its integer displacement, widened by the six-tap footprint -- 2
//           before, 3 after -- in a direction whose vector component has a fractional part (dec_luma_frac);
//   chroma  the block's 2x2 samples c .. c+1 and the right / lower neighbour c+2, which the bilinear form
//           reads whatever the fraction (weight 0 for a whole-sample component).
// For a whole-sample component the chroma window binds on the far side (p <= 35: one less than luma alone),
// for a fractional one the luma footprint (p - 2 >= -24, p + 6 <= 39).
// Lane-parallel (block lane & 15 per lane), whole wave: call with every lane active.
DEV bool mb_in_window(const MbInfo &I) {
    const int b = threadIdx.x & 15;
    const uint32_t mv = ((const uint32_t *)I.mv)[b];
    const int mvx = (int16_t)(mv & 0xffff), mvy = (int16_t)(mv >> 16);
    const int x = (b & 3) * 4 + (mvx >> 2), y = (b >> 2) * 4 + (mvy >> 2);
    const int fx = (mvx & 3) != 0, fy = (mvy & 3) != 0;
    const int cx = (b & 3) * 2 + (mvx >> 3), cy = (b >> 2) * 2 + (mvy >> 3);
    const bool okl = min(x - 2 * fx, y - 2 * fy) >= DWIN_LO && max(x + 3 * fx, y + 3 * fy) + 3 < DWIN_HI;
    const bool okc = min(cx, cy) >= DWINC_LO && max(cx, cy) + 2 < DWINC_HI;
    return __ballot(!(okl && okc)) == 0;
}

// Tickets [0, S*mbh) reconstruct MB rows; tickets [S*mbh, 2*S*mbh) are the deblocking rows that
// trail them, fed by the 128 granules per MB the reconstruction rows publish (deblock.inc); they only
// wait on lower tickets, so dispatch order and residency limits cannot deadlock.
#ifdef H264MI_REC_WPE  // diagnostics: occupancy target (waves per SIMD) for A/B builds
#define H264MI_REC_WPE_ATTR __attribute__((amdgpu_waves_per_eu(H264MI_REC_WPE, H264MI_REC_WPE)))
#else
#define H264MI_REC_WPE_ATTR
#endif
// PRE: the records are resolved (dec_resolve_kernel ran over the call): the MB loop neither waits for nor
// publishes granules 8..12 and calls no rule function; only an intra MB waits for the row above (its samples).
template <bool PRE> DEV void dec_recon_body(const DecLaunch &a) {
    __shared__ union { DecLds r; DbkLds d; } SH;
    DecLds &S = SH.r;
    __shared__ int s_ticket;
#ifndef H264MI_REC_RELANE  // lane re-read at every use (e_tid, enc_mb.inc): 233 -> 163 VGPRs, 3 waves per SIMD
#define H264MI_REC_RELANE 1   // instead of 2. Round 3 measured it within noise (profiles/round3/ab_relane); round 4,
#endif                        // with the lighter row hand-off, +1.2 % in three A/B pairs (profiles/round4/ab_recon_relane.txt)
#if H264MI_REC_RELANE
#define lane (e_tid() & 63)
#else
    const int lane = threadIdx.x;
#endif
    if (lane == 0) s_ticket = (int)atomicAdd(a.ticket, 1u);
    wave_lds_sync();
    const int t = uni(s_ticket), nrows = a.S * a.mbh;
    if (t >= nrows) {  // deblocking row
        const int u = t - nrows, dby = u / a.S, dsi = u % a.S;
        if (dby >= a.mbh) return;
        CONSTANT const DbkDesc &DD = cst(a.dbk)[dsi];
        if (DD.active && uni(*DD.active) == 0) return;
        const DbkLaunch dl{a.mbw, a.mbh, a.S, a.dbk, nullptr, nullptr};
        deblock_row(SH.d, dl, DD, dby, DbkSrcGranules{gbl((const uint64_t *)DD.src_gran), a.mbw, dby, (uint32_t)uni((int)*DD.epoch)});
        return;
    }
    const int mby = t / a.S, sidx = t % a.S;
    CONSTANT const DecDesc &D = cst(a.desc)[sidx];
    DecState *st = D.st;
    if (!uni(st->got_pic)) return;
    const uint32_t epoch = (uint32_t)uni((int)st->epoch);
    const int par = uni(st->parity) & 1;
    const bool has_ref = uni(st->has_ref) != 0;  // the padded planes of pic[par] are valid
    const Xf XF = xf_consts(lane & 15);          // lane constants of the 4x4 transforms
    GLOBAL const uint8_t *R0 = gbl(D.pic[par][0]), *R1 = gbl(D.pic[par][1]), *R2 = gbl(D.pic[par][2]);
    GLOBAL uint32_t *info32 = gbl((uint32_t *)D.info);
    GLOBAL const MbCoef *coefg = gbl((const MbCoef *)D.coef);
    GLOBAL uint64_t *egr = gbl(D.egran);
    int32_t *abort_word = &st->err;
    if (!PRE && a.streamed && !prog_wait(gbl(&D.frm->prog), a.tag, (uint32_t)mby + 1, abort_word)) return;
    const int mbw = a.mbw, cw = mbw * 16, ch = a.mbh * 16, ccw = cw / 2, cch = ch / 2;
    const int Y = mby * 16;
    GLOBAL uint64_t *grow_prev = gbl(D.gran) + (size_t)(mby > 0 ? mby - 1 : 0) * mbw * H264MI_GRANULES_PER_MB;
    GLOBAL uint64_t *grow = gbl(D.gran) + (size_t)mby * mbw * H264MI_GRANULES_PER_MB;
    const int Y0 = Y + DWIN_LO;
    static_assert(DWIN_HI - DWIN_LO == DWIN_ROWS && DWIN_ROWS == 64 && WIN_RING == 64, "one window row per lane, 64-column ring");
    static_assert(-DWIN_LO <= H264MI_LPADY && DWIN_HI - 16 <= H264MI_LPADY && -DWIN_LO <= H264MI_LPADX && DWIN_HI - 16 <= H264MI_LPADX,
                  "the window of an edge macroblock lies inside the plane's padding");
    // ---- one MB ahead: the MB record and coefficient image (written by the parse launch) and the
    // reference window strips (enc_mb.inc window layout; lane -> 1 luma strip + 1 chroma strip)
    GLOBAL const uint8_t *plw = gbl((const uint8_t *)D.pl) + (ptrdiff_t)(Y0 + lane) * D.ps;
    GLOBAL const uint8_t *plcw = gbl((const uint8_t *)D.plc[lane >> 5]) + (ptrdiff_t)(mby * 8 - 12 + (lane & 31)) * D.psc;
    uint32_t pf_info = 0, pf_cf[4] = {0, 0, 0, 0};
    u32x4 pf_w = {0, 0, 0, 0};
    u32x2 pf_c = {0, 0};
    auto issue = [&](int mx) {
        const int mi = mby * mbw + mx;
        if (lane < 32) pf_info = info32[(size_t)mi * 32 + lane];
        GLOBAL const uint32_t *cf32 = (GLOBAL const uint32_t *)(coefg + mi);
#pragma unroll
        for (int k = 0; k < 4; k++) if (lane + 64 * k < 208) pf_cf[k] = cf32[lane + 64 * k];
        if (has_ref && mx > 0) {
            pf_w = *(GLOBAL const u32x4 *)(plw + 16 * mx + 24);
            pf_c = *(GLOBAL const u32x2 *)(plcw + 8 * mx + 12);
        }
    };
    if (has_ref) {  // initial window: luma columns [-24, 40), chroma [-12, 20)
#pragma unroll
        for (int j = 0; j < 4; j++) *(u32x4 *)&S.win[lane * WIN_RING + 16 * j] = *(GLOBAL const u32x4 *)(plw - 24 + 16 * j);
#pragma unroll
        for (int j = 0; j < 4; j++) *(u32x2 *)&S.winc[lane >> 5][(lane & 31) * WINC_RING + 8 * j] = *(GLOBAL const u32x2 *)(plcw - 12 + 8 * j);
    }
    issue(0);
    // section timer (a.prof, env H264MI_RECON_PROF): 1 prefetch, 2 row-above wait, 3 record resolution,
    // 4 levels + context, 5 residuals, 6 luma prediction, 7 chroma, 8 outputs + window slide
    uint64_t t_prev = a.prof ? clock64() : 0, s_prof[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    auto lap = [&](int k) { if (a.prof) { const uint64_t tt = clock64(); s_prof[k] += tt - t_prev; t_prev = tt; } };

    int pix_next = 0;  // the row above's MBs below this index have their samples in S.gp
    for (int mbx = 0; mbx < mbw; mbx++) {
        const int X = mbx * 16, mbi = mby * mbw + mbx;
        if (lane < 32) ((uint32_t *)&S.info)[lane] = pf_info;
        // the record's type word and slice word in scalars (no LDS round trip on the row-to-row chain)
        const uint32_t rw0 = __builtin_amdgcn_readfirstlane(pf_info), rw31 = __builtin_amdgcn_readlane(pf_info, 31);
        const int rt = (int)(rw0 & 255);
        {  // the coefficient image only for an MB that reads it (I_16x16 always has its DC block, I_PCM its samples)
            if (rt == MI_I16 || rt == MI_IPCM || ((rw0 >> 16) & 255) != 0) {
#pragma unroll
                for (int k = 0; k < 4; k++) if (lane + 64 * k < 208) S.cf[lane + 64 * k] = pf_cf[k];
            }
        }
        if (mbx + 1 < mbw) issue(mbx + 1);  // MB x+1's record/coefficients and window strip (committed at the end of MB x)
        lap(1);
        // The row above hands over two granule groups per MB: its resolved vectors / type / Intra4x4 modes
        // (granules 8..12) right after its record resolution, its bottom sample rows (0..7) after its
        // reconstruction. Every MB needs the first group of (x+1, y-1) (vector and mode prediction); only
        // an intra MB needs the samples of (x-1..x+1, y-1), so inter MBs follow the row above at the
        // distance of its record resolution, not of its whole reconstruction.
        if (!PRE && mby > 0) {
            uint32_t v;
            if (mbx == 0) {
                if (!gran_wait(grow_prev + 8, 5, epoch, &v, abort_word)) return;
                if (lane < 5) S.gm[0][lane] = v;
            }
            if (mbx + 1 < mbw) {
                if (!gran_wait(grow_prev + (size_t)(mbx + 1) * H264MI_GRANULES_PER_MB + 8, 5, epoch, &v, abort_word)) return;
                if (lane < 5) S.gm[(mbx + 1) % 3][lane] = v;
            }
        }
        wave_lds_sync();
        if (mby > 0 && (rt == MI_I4 || rt == MI_I16)) {
            const int j1 = mbx + 1 < mbw ? mbx + 1 : mbx;
            for (int j = max(pix_next, mbx - 1); j <= j1; j++) {
                uint32_t v;
                if (!gran_wait(grow_prev + (size_t)j * H264MI_GRANULES_PER_MB, 8, epoch, &v, abort_word)) return;
                if (lane < 8) S.gp[j % 3][lane] = v;
            }
            pix_next = j1 + 1;
            wave_lds_sync();
        }
        lap(2);
        // neighbour availability by slice: the record's slice word carries its slice's first MB
        const uint32_t nbm = uni(mb_nb_mask(mbx, mby, mbw, MB_SLICE_FIRST(rw31)));
        if (PRE) {
        } else if (rt == MI_PSKIP || rt == MI_P16x16) {
            // one vector for the whole MB: the row below's granules straight from the scalar (record default
            // Intra4x4 modes 2, as the parse writes every non-I4 record), ahead of the LDS copy
            const uint32_t mvw = resolve_p16_uni(S, mbx, nbm, rt == MI_PSKIP);
            if (lane >= 8 && lane < 13)
                gran_store(grow + (size_t)mbx * H264MI_GRANULES_PER_MB + lane, epoch, lane < 12 ? mvw : (uint32_t)rt | 0x222200u);
            wave_lds_sync();
        } else {
            if (lane == 0) resolve_record(S, mbx, nbm);
            wave_lds_sync();
        }
        if (!PRE && lane >= 8 && lane < 13 && !(rt == MI_PSKIP || rt == MI_P16x16)) {  // vectors of the bottom blocks, type and bottom Intra4x4 modes -> the row below
            const MbInfo &R = S.info;
            const uint32_t v = lane < 12 ? ((const uint32_t *)R.mv)[12 + lane - 8] : res_type_word(R);
            gran_store(grow + (size_t)mbx * H264MI_GRANULES_PER_MB + lane, epoch, v);
        }
        if (lane < 32) gran_store(egr + (size_t)mbi * 128 + 96 + lane, epoch, ((const uint32_t *)&S.info)[lane]);  // -> deblocking row
        const MbInfo &I = S.info;
        const int type = I.type;
        const bool intra = type == MI_I4 || type == MI_I16, ipcm = type == MI_IPCM;
        lap(3);
        // ---- levels stay in S.cf (only blocks with TotalCoeff > 0 were stored; the residual stage
        // masks the others); I_PCM samples are the record's payload
        const MbCoef &CF = *(const MbCoef *)S.cf;
        const uint8_t *PCM = (const uint8_t *)&CF;  // the record's payload, in S.cf
        // ---- neighbour pixels: intra prediction only (an inter MB never waited for the row above's samples,
        // so S.gp may be stale then; S.left / S.leftc are rewritten by every MB's outputs)
        const bool has_top = nbm & NB_B, has_left = nbm & NB_A, has_tr = nbm & NB_C, has_tl = nbm & NB_D;
        const uint32_t *PB = S.gp[mbx % 3], *PC = S.gp[(mbx + 1) % 3], *PD = S.gp[(mbx + 2) % 3];
        if (intra) {
        if (lane < 21) {
            int v = 0;
            if (lane == 0) v = has_tl ? (PD[3] >> 24) & 255 : 0;
            else if (lane <= 16) v = has_top ? (PB[(lane - 1) >> 2] >> (8 * ((lane - 1) & 3))) & 255 : 0;
            else v = has_tr ? (PC[(lane - 17) >> 2] >> (8 * ((lane - 17) & 3))) & 255 : 0;
            S.top[lane] = (uint8_t)v;
        }
        if (lane >= 32 && lane < 50) {
            int pl = (lane - 32) / 9, k = (lane - 32) % 9, v = 0;
            if (k == 0) v = has_tl ? (PD[5 + 2 * pl] >> 24) & 255 : 0;
            else v = has_top ? (PB[4 + 2 * pl + ((k - 1) >> 2)] >> (8 * ((k - 1) & 3))) & 255 : 0;
            S.topc[pl][k] = (uint8_t)v;
        }
        if (!has_left && lane < 16) { S.left[lane] = 0; S.leftc[lane >> 3][lane & 7] = 0; }
        }
        wave_lds_sync();
        lap(4);
        // ---- residuals (8.5.10-8.5.12), lane per coefficient: four 4x4 blocks per pass (blocks
        // 0..15 luma raster, 16..23 Cb/Cr), DPP inverse transform (h264mi_dev.h xf_inv). Passes whose
        // blocks carry no level and no DC are skipped; P_Skip macroblocks have no residual at all.
        const bool has_res = type != MI_PSKIP && !ipcm;
        if (has_res) {
            const QuantQP ql = make_qqp(I.qp), qcc = make_qqp(I.qpc);
            const bool i16 = type == MI_I16;
            const bool cdc_any = (I.cbp >> 4) != 0;
            if (lane < 16 && i16) S.dcval[lane] = luma_dc_scale(xf_had(CF.lumadc[XF.zz], XF), ql);  // 8.5.10
            if (lane >= 16 && lane < 24) {  // 8.5.11
                const int pl = (lane - 16) >> 2, k = (lane - 16) & 3;
                const int a0 = cdc_any ? CF.cdc[pl][0] : 0, b0 = cdc_any ? CF.cdc[pl][1] : 0;
                const int e0 = cdc_any ? CF.cdc[pl][2] : 0, g0 = cdc_any ? CF.cdc[pl][3] : 0;
                const int f = k == 0 ? a0 + b0 + e0 + g0 : k == 1 ? a0 - b0 + e0 - g0 : k == 2 ? a0 + b0 - e0 - g0 : a0 - b0 - e0 + g0;
                S.dcval[16 + 4 * pl + k] = ((f * qcc.v0) << qcc.q6) >> 1;
            }
            wave_lds_sync();
#pragma unroll 1
            for (int pass = 0; pass < 6; pass++) {
                const int blk = 4 * pass + (lane >> 4), pos = lane & 15;
                const bool luma = pass < 4;
                const int nz = I.nnz[blk];
                const bool dc = luma ? i16 : cdc_any;
                if (__ballot(nz != 0 || dc) == 0) { S.res[blk][pos] = 0; continue; }  // uniform
                const int16_t *lv = luma ? CF.luma[blk] : CF.cac[(blk - 16) >> 2][(blk - 16) & 3];
                const int first = (luma && !i16) ? 0 : 1;  // I16 and chroma blocks: AC levels only
                const int level = (nz && pos >= first) ? lv[XF.zz] : 0;
                // field-wise selects: a reference to ql or qcc chosen per pass would copy both through scratch
                const int vl = XF.cls == 0 ? ql.v0 : (XF.cls == 1 ? ql.v1 : ql.v2), vc = XF.cls == 0 ? qcc.v0 : (XF.cls == 1 ? qcc.v1 : qcc.v2);
                int w = (level * (luma ? vl : vc)) << (luma ? ql.q6 : qcc.q6);
                if (pos == 0 && dc) w = S.dcval[blk];
                S.res[blk][pos] = (int16_t)((xf_inv(w, XF) + 32) >> 6);
            }
        }
        wave_lds_sync();
        lap(5);
        // ---- luma prediction + reconstruction
        const bool inwin = has_ref && !intra && !ipcm && mb_in_window(I);  // once for luma and chroma, whole wave
        if (ipcm) {
            for (int i = lane; i < 256; i += 64) S.rec[i] = PCM[i];
            for (int i = lane; i < 128; i += 64) S.recc[i >> 6][i & 63] = PCM[256 + i];
        } else if (type == MI_I4) {
            for (int blk = 0; blk < 16; blk++) {
                const int ras = BLK2RAS[blk], bx = ras & 3, by = ras >> 2, ox = bx * 4, oy = by * 4;
                const bool bt = by > 0 || has_top, bl = bx > 0 || has_left;
                bool btr;
                if (by == 0) btr = bx < 3 ? has_top : has_tr;
                else btr = (bx < 3) && ras != 5 && ras != 13;
                if (lane < 13) {
                    int v = 0;
                    if (lane == 0) {
                        if (bt && bl) v = (bx > 0 && by > 0) ? S.rec[(oy - 1) * 16 + ox - 1] : (by > 0 ? S.left[oy - 1] : S.top[ox]);
                    } else if (lane <= 8) {
                        int i = lane - 1;
                        if (bt) { int ii = (i >= 4 && !btr) ? 3 : i; v = by > 0 ? S.rec[(oy - 1) * 16 + ox + ii] : S.top[1 + ox + ii]; }
                    } else {
                        int i = lane - 9;
                        if (bl) v = bx > 0 ? S.rec[(oy + i) * 16 + ox - 1] : S.left[oy + i];
                    }
                    S.n4[lane] = (uint8_t)v;
                }
                wave_lds_sync();
                if (lane < 16) {
                    const int m = I.i4mode[ras];
                    int s4t = S.n4[1] + S.n4[2] + S.n4[3] + S.n4[4], s4l = S.n4[9] + S.n4[10] + S.n4[11] + S.n4[12];
                    int dcv = (bt && bl) ? (s4t + s4l + 4) >> 3 : bl ? (s4l + 2) >> 2 : bt ? (s4t + 2) >> 2 : 128;
                    int pv = m == 2 ? dcv : i4_tap_eval(c_I4.t[m][lane], S.n4);
                    S.rec[(oy + (lane >> 2)) * 16 + ox + (lane & 3)] = (uint8_t)clip1(pv + S.res[ras][lane]);
                }
                wave_lds_sync();
            }
        } else if (type == MI_I16) {
            const I16Ctx k16 = i16_ctx(S, has_top, has_left);
            for (int i = lane; i < 256; i += 64) {
                int x = i & 15, y = i >> 4, ras = (y >> 2) * 4 + (x >> 2);
                S.rec[i] = (uint8_t)clip1(i16_pred(S, k16, I.i16mode, x, y) + S.res[ras][(y & 3) * 4 + (x & 3)]);
            }
        } else if (inwin) {
            // inter from the G window: a macroblock of whole-sample vectors (wave-uniform) reads its samples and
            // nothing else; any other runs the six-tap filters its blocks need (dec_luma_frac)
            {  // one row of four samples of one 4x4 block per lane (one vector per block)
                const int y = lane >> 2, x0 = (lane & 3) * 4, ras = (y >> 2) * 4 + (x0 >> 2);
                const int mx = I.mv[ras][0], my = I.mv[ras][1];
                const int idx = (my & 3) * 4 + (mx & 3);
                const int gx = X + x0 + (mx >> 2), wr = Y + y + (my >> 2) - Y0;
                uint32_t pv;
                if (__ballot(idx != 0) == 0) pv = dwin4(S, wr, gx);
                else pv = dec_luma_frac(S, wr, gx, idx);
                uint32_t o = 0;
                if (has_res) {
                    const u32x2 r2 = *(const u32x2 *)&S.res[ras][(y & 3) * 4];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int rj = (int16_t)(((j < 2 ? r2.x : r2.y) >> (16 * (j & 1))) & 0xffff);
                        o |= (uint32_t)clip1((int)((pv >> (8 * j)) & 255) + rj) << (8 * j);
                    }
                } else o = pv;
                *(uint32_t *)&S.rec[y * 16 + x0] = o;
            }
        } else {
            // inter with a block outside the window (or no window): interpolation from the deblocked picture
            const GlobGet gg{R0, cw, ch};
            for (int i = lane; i < 256; i += 64) {
                int x = i & 15, y = i >> 4, ras = (y >> 2) * 4 + (x >> 2);
                int mx = I.mv[ras][0], my = I.mv[ras][1];
                int gx = X + x + (mx >> 2), gy = Y + y + (my >> 2);
                int pv = qpel(gg, gx, gy, mx & 3, my & 3);
                S.rec[i] = (uint8_t)clip1(pv + (has_res ? S.res[ras][(y & 3) * 4 + (x & 3)] : 0));
            }
        }
        lap(6);
        // ---- chroma prediction + reconstruction
        if (!ipcm) {
            if (intra) {
                const CCtx kc = chroma_ctx(S, has_top, has_left);
                for (int i = lane; i < 128; i += 64) {
                    int pl = i >> 6, p = i & 63, x = p & 7, y = p >> 3;
                    int dv = chroma_dc_blk(S, kc, pl, x >> 2, y >> 2);
                    int pv = chroma_pred(S, kc, I.cmode, pl, x, y, dv);
                    S.recc[pl][p] = (uint8_t)clip1(pv + S.res[16 + 4 * pl + (y >> 2) * 2 + (x >> 2)][(y & 3) * 4 + (x & 3)]);
                }
            } else if (inwin) {
                // sample p of both planes per lane: one vector read, the eight window samples and two residuals
                // in flight together (the two planes as two passes re-read the vector behind the first pass's
                // stores, which the compiler cannot prove disjoint from S.info)
                const int p = lane, x = p & 7, y = p >> 3, ras = (y >> 1) * 4 + (x >> 1);
                const int mx = I.mv[ras][0], my = I.mv[ras][1], fx = mx & 7, fy = my & 7;
                const int cx = mbx * 8 + x + (mx >> 3), r0 = (y + (my >> 3) + 12) * WINC_RING, r1 = r0 + WINC_RING;
                const int c0 = (cx + 12) & 31, c1 = (cx + 13) & 31;
                const int w00 = (8 - fx) * (8 - fy), w01 = fx * (8 - fy), w10 = (8 - fx) * fy, w11 = fx * fy;
                const int rb = (y >> 2) * 2 + (x >> 2), ri = (y & 3) * 4 + (x & 3);
                int pv[2], rs[2];
#pragma unroll
                for (int pl = 0; pl < 2; pl++) {
                    const uint8_t *Wc = S.winc[pl];
                    pv[pl] = (w00 * Wc[r0 + c0] + w01 * Wc[r0 + c1] + w10 * Wc[r1 + c0] + w11 * Wc[r1 + c1] + 32) >> 6;
                    rs[pl] = has_res ? S.res[16 + 4 * pl + rb][ri] : 0;
                }
#pragma unroll
                for (int pl = 0; pl < 2; pl++) S.recc[pl][p] = (uint8_t)clip1(pv[pl] + rs[pl]);
            } else {
                for (int i = lane; i < 128; i += 64) {
                    int pl = i >> 6, p = i & 63, x = p & 7, y = p >> 3;
                    int ras = (y >> 1) * 4 + (x >> 1);
                    int mx = I.mv[ras][0], my = I.mv[ras][1];
                    int fx = mx & 7, fy = my & 7, gx = mbx * 8 + x + (mx >> 3), gy = mby * 8 + y + (my >> 3);
                    GLOBAL const uint8_t *Rp = pl ? R2 : R1;
                    int xa = clip3(0, ccw - 1, gx), xb = clip3(0, ccw - 1, gx + 1), ya = clip3(0, cch - 1, gy), yb = clip3(0, cch - 1, gy + 1);
                    int A = Rp[ya * ccw + xa], B = Rp[ya * ccw + xb], C = Rp[yb * ccw + xa], E = Rp[yb * ccw + xb];
                    int pv = ((8 - fx) * (8 - fy) * A + fx * (8 - fy) * B + (8 - fx) * fy * C + fx * fy * E + 32) >> 6;
                    S.recc[pl][p] = (uint8_t)clip1(pv + (has_res ? S.res[16 + 4 * pl + (y >> 2) * 2 + (x >> 2)][(y & 3) * 4 + (x & 3)] : 0));
                }
            }
        }
        wave_lds_sync();
        lap(7);
        // ---- outputs: unfiltered MB to the deblocking row, hand-off granules, left state
        gran_store(egr + (size_t)mbi * 128 + lane, epoch, ((const uint32_t *)S.rec)[lane]);
        if (lane < 32) gran_store(egr + (size_t)mbi * 128 + 64 + lane, epoch, ((const uint32_t *)S.recc[lane >> 4])[((lane >> 1) & 7) * 2 + (lane & 1)]);
        if (lane < 8) {  // bottom sample rows -> the row below (its intra MBs)
            const uint32_t v = lane < 4 ? ((const uint32_t *)S.rec)[60 + lane] : ((const uint32_t *)S.recc[(lane - 4) >> 1])[14 + (lane & 1)];
            gran_store(grow + (size_t)mbx * H264MI_GRANULES_PER_MB + lane, epoch, v);
        }
        if (lane < 16) { S.left[lane] = S.rec[lane * 16 + 15]; S.leftc[lane >> 3][lane & 7] = S.recc[lane >> 3][(lane & 7) * 8 + 7]; }
        if (!PRE && lane < 32) ((uint32_t *)&S.linfo)[lane] = ((const uint32_t *)&S.info)[lane];
        if (has_ref && mbx + 1 < mbw) {  // slide the window: MB x+1's new strip (columns X+40..X+55)
            const int nx = mbx + 1;
            *(u32x4 *)&S.win[lane * WIN_RING + ((16 * nx + 48) & 63)] = pf_w;
            *(u32x2 *)&S.winc[lane >> 5][(lane & 31) * WINC_RING + ((8 * nx + 24) & 31)] = pf_c;
        }
        wave_lds_sync();
        lap(8);
    }
    if (a.prof && lane == 0) {
#pragma unroll
        for (int k = 1; k < 9; k++) atomicAdd((unsigned long long *)&a.prof[k], (unsigned long long)s_prof[k]);
    }
#if H264MI_REC_RELANE
#undef lane
#endif
}
__global__ __launch_bounds__(64) H264MI_REC_WPE_ATTR void dec_recon_kernel(DecLaunch a) { dec_recon_body<false>(a); }
__global__ __launch_bounds__(64) H264MI_REC_WPE_ATTR void dec_recon_pre_kernel(DecLaunch a) { dec_recon_body<true>(a); }

// after reconstruction + loop filter: flip the picture ping-pong and mark a reference available
// check: streamed reconstruction -- the picture's final decision first (dec_frame_check, dec_parse.inc)
struct DecEndLaunch { int S; const DecDesc *desc; int check; };
__global__ void dec_end_kernel(DecEndLaunch a) {
    int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.S) return;
    if (a.check) dec_frame_check(a.desc[s]);
    DecState *st = a.desc[s].st;
    // the new picture is pic[parity ^ 1]; a reference picture becomes the reference, a non-reference one
    // (nal_ref_idc 0) is only output
    if (st->got_pic) {
        st->outpar = st->parity ^ 1;
        if (!st->nonref) { st->parity ^= 1; st->has_ref = 1; }
    }
}

// Per-frame output of a batched call (after dec_end_kernel of frame f): the picture just produced,
// cropped by its SPS (frame_cropping, as the C-ABI read-out) into the caller's tight I420 buffer
// in[s].out, and 1 / 0 into in[s].got (0: no picture -- a damaged access unit, or no reference). Grid
// (row groups, S): 4 rows of the 2H output rows (Y, then U, then V) per 256-thread block, 64 lanes a row.
struct DecOutLaunch { int S, cw, ch; const DecDesc *desc; const DecInput *in; };  // desc / in: frame f's S entries
__global__ __launch_bounds__(256) void dec_output_kernel(DecOutLaunch a) {
    const int s = blockIdx.y;
    if (s >= a.S) return;
    const DecState *st = a.desc[s].st;
    const DecInput &I = a.in[s];
    const int ok = st->got_pic && !st->err;
    if (I.got && blockIdx.x == 0 && threadIdx.x == 0) *I.got = ok;
    if (!ok || !I.out) return;
    const int c0 = st->ps.crop[0], c1 = st->ps.crop[1], c2 = st->ps.crop[2], c3 = st->ps.crop[3];
    const int W = a.cw - 2 * (c0 + c1), H = a.ch - 2 * (c2 + c3), x0 = 2 * c0, y0 = 2 * c2;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= 2 * H || W <= 0 || H <= 0) return;
    const uint8_t *const *pic = a.desc[s].pic[st->outpar & 1];
    const uint8_t *src;
    uint8_t *dst;
    int n;
    if (r < H) { src = pic[0] + (size_t)(y0 + r) * a.cw + x0; dst = I.out + (size_t)r * W; n = W; }
    else {
        const int q = r - H, pl = 1 + q / (H / 2), y = q % (H / 2);
        src = pic[pl] + (size_t)(y0 / 2 + y) * (a.cw / 2) + x0 / 2;
        dst = I.out + (size_t)W * H + (size_t)(pl - 1) * (W / 2) * (H / 2) + (size_t)y * (W / 2);
        n = W / 2;
    }
    for (int x = lane; x < n; x += 64) dst[x] = src[x];
}

}  // namespace h264mi
