// runtime_dec.inc -- host runtime of the decoder: HBM allocation and the per-call launch sequence
//   dec_parse_kernel -> dec_resolve_kernel -> dec_recon_pre_kernel (+ deblocking rows) -> dec_end_kernel
//   (a streamed call: dec_parse_kernel -> dec_recon_kernel, which resolves the records itself;
//    with slice-copy concealment on: dec_parse_kernel -> dec_conceal_kernel -> the rest, never streamed)
namespace h264mi {

constexpr int DEC_PSTREAMS = 3;      // default parse streams: consecutive calls rotate (each wants its own HW queue:
                                     // GPU_MAX_HW_QUEUES >= 6 beside an encoder and a caller stream)
struct DecCtx {
    int mbw, mbh, nmb, cw, ch, S, B;   // B = frames per stream one call may carry
    int NG;                            // slot groups of B frames (ring); a call takes the next group
    hipStream_t stream;                // reconstruction stream (the caller's)
    bool own_stream;
    static constexpr int PMAX = 16;
    int np = DEC_PSTREAMS;             // parse streams in use (h264mi_dec_set_parse_streams)
    hipStream_t pst[PMAX] = {};        // scan + header + slice-data kernels
    int cu_lo = 0, cu_hi = 0;          // parse streams' CU mask bits (lo == hi: none)
    std::vector<hipEvent_t> ev_hdr, ev_parsed, ev_recon;  // per slot group
    hipEvent_t ev_in = nullptr;        // caller-stream tail at call time (inputs ready, default ordering)
    int grp = 0;                       // slot group used by the next call
    uint32_t calls = 0;                // header-chain parity
    uint8_t *d_pool = nullptr;
    size_t pool_bytes = 0;             // device bytes held (pool; the C-ABI staging buffers are added on use)
    DecState *d_st = nullptr;
    DecDesc *d_desc = nullptr;          // [NG*B][S]: frame slot f of stream s at f * S + s
    DbkDesc *d_dbk = nullptr;           // [NG*B][S]
    PlanesDesc *d_pd = nullptr;         // [S] reference planes of each stream
    DecInput *d_in = nullptr;           // [NG*B][S] access units (per slot)
    uint32_t *d_ticket = nullptr;       // 2 per frame slot (reconstruction, deblocking)
    // record resolution ahead of the reconstruction (dec_resolve_kernel), for every call that is not streamed:
    // one launch per call on its parse stream, behind the slice data (the reserved parse CUs; one launch per
    // frame on the reconstruction stream gained nothing, profiles/dec_preresolve/placement_ab.txt). 0: never
    // (the in-wavefront build, as a streamed call). Env H264MI_DEC_RESOLVE at creation, h264mi_dec_set_resolve.
    int resolve = 1;
    // slice-copy concealment of lost slices (DESIGN.md §6.5; h264mi_dec_set_conceal, the C-ABI slots: env
    // H264MI_DEC_CONCEAL=1): each call captures it when it is enqueued. While it is on no call is streamed (the gaps
    // are known only once every slice is parsed); `streamed` keeps the mode that returns when it is turned off.
    int conceal = 0;
    int32_t *d_conc = nullptr;          // [B][S] concealed MBs of the frames of the last call (dec_frame_begin_kernel)
    int last_n = 0;                     // frames of the last call
    long long resolve_launches = 0;
    uint32_t *d_rticket = nullptr;      // its ticket counters, never reset: one per slot group (a group's launches are
    uint32_t rt_base[16] = {};          // ordered by ev_recon); the value each has before its next launch
    std::vector<DecDesc> h_desc;
    DecInput *h_in = nullptr;           // pinned: a pageable source would make hipMemcpyAsync block the
                                        // host until the parse stream reached the copy
    size_t lds_bytes = 0, lds_min = 0;  // slice-data launch LDS (padded on a reserved lane, dec_set_parse_cus)
    int slice_waves = 1;                // slice-data waves per frame (a multi-slice picture's slices in parallel)
    // streamed reconstruction (DESIGN.md §6): the first frame of a call is reconstructed behind its slice
    // data, row by row, instead of after the parse launch. Its row waves wait on the GPU for the parse, so
    // they must never keep the parse waves from a CU: automatic only while every streamed decoder's waves
    // together fit in STREAMED_WAVES (the rest of the GPU stays free for the parse), or forced by a caller
    // whose reconstruction stream is kept off the parse CUs (h264mi_dec_set_streamed)
    int streamed = 0;
    int streamed_auto = 0;              // waves counted in g_streamed_waves
    int gate_rows = 0;                  // streamed, forced: the reconstruction launch waits (dec_gate_kernel) until
                                        // every stream has this many MB rows parsed (0: no gate)
    // next call only (h264mi_dec_set_recon_gate): frame f < rg_count of the call reconstructs after *rg_counter
    // reaches rg_target + f * rg_step (dec_wait_counter_kernel, bounded by rg_limit ticks of 10 ns)
    const uint32_t *rg_counter = nullptr;
    uint32_t rg_target = 0, rg_step = 0, rg_limit = 0;
    int rg_count = 0;
    int out_fmt = 0;                    // H264MI_FMT_*: what the next calls write to their d_out buffers
    int w = 0, h = 0;                   // the size the batch decoder was created with (0: a C-ABI decoder)
    bool out_lay_set = false;           // a layout instead (h264mi_dec_set_output_layout), good for w x h
    h264mi_pix_layout out_lay = {};
    h264mi_colorspec out_cs = {};       // what H264MI_FMT_RGBA output converts under (h264mi_dec_set_output_colorspec); all 0: color.inc's kernel
    // C-ABI staging
    uint8_t *d_nal = nullptr;
    size_t nal_cap = 0;
    uint8_t *d_rgba = nullptr;
    size_t rgba_cap = 0;
    uint8_t *d_tight = nullptr;  // C-ABI read-out: the cropped tight I420 picture (dec_output_kernel), one copy to the host
    size_t tight_cap = 0;
    uint64_t *d_prof = nullptr;  // parse section counters (env H264MI_PARSE_PROF=1), 16 per frame slot
    uint64_t *d_rprof = nullptr; // reconstruction section counters (env H264MI_RECON_PROF=1), 16 totals
    // optional HIP-event timing for bench.py: [0] the reconstruction launch (decoder stream), [1] dec_parse_kernel and
    // the resolution pass behind it (parse streams)
    bool timing = false;
    std::vector<hipEvent_t> tev[2];
    int tev_used[2] = {0, 0};
};
static std::atomic<int> g_streamed_waves{0};
// Automatic streaming's wave budget: a quarter of dec_recon_kernel's resident wave slots on this device (CUs x
// the one-wave blocks per CU hipOccupancyMaxActiveBlocksPerMultiprocessor reports for it, which accounts for
// its VGPRs), so the waiting reconstruction waves of all automatically streamed decoders of the process can
// never hold every CU a parse wave needs -- on a partitioned or smaller GPU too. Computed on first use;
// h264mi_dec_set_streamed_budget overrides it (tests). Other processes sharing the GPU are not counted.
static std::atomic<int> g_streamed_budget{0};
static int dec_streamed_budget() {
    int b = g_streamed_budget.load();
    if (b > 0) return b;
    int dev = 0, cus = 0, blocks = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, dec_recon_kernel, 64, 0) != hipSuccess)
        return 0;  // unknown device: no automatic streaming
    b = cus * blocks / 4;
    g_streamed_budget.store(b);
    return b;
}
static void dec_streamed_release(DecCtx *c) {
    if (c->streamed_auto) g_streamed_waves.fetch_sub(c->streamed_auto);
    c->streamed_auto = 0;
    c->streamed = 0;
}
// mode 1: on (the caller keeps the reconstruction stream off the parse CUs), 0: off, -1: automatic
static int dec_set_streamed(DecCtx *c, int mode) {
    if (mode < -1 || mode > 1) return -1;
    dec_streamed_release(c);
    c->gate_rows = 0;
    if (mode == 1) { c->streamed = 1; c->gate_rows = (3 * c->mbh) / 4; }
    else if (mode == -1) {
        const int w = 2 * c->S * c->mbh;  // reconstruction + deblocking row waves of one launch
        if (g_streamed_waves.fetch_add(w) + w <= dec_streamed_budget()) { c->streamed = 1; c->streamed_auto = w; }
        else g_streamed_waves.fetch_sub(w);
    }
    return 0;
}
static hipError_t dec_sync_all(DecCtx *c) {
    hipError_t e = hipStreamSynchronize(c->stream);
    for (int i = 0; i < DecCtx::PMAX; i++)
        if (c->pst[i] && e == hipSuccess) e = hipStreamSynchronize(c->pst[i]);
    return e;
}
// bracket one launch of kernel class k (0 recon, 1 parse) on stream st with timing events
static int dec_time_mark(DecCtx *c, int k, hipStream_t st) {
    if (!c->timing) return 0;
    if (c->tev_used[k] + 1 > (int)c->tev[k].size())
        for (int i = 0; i < 64; i++) { hipEvent_t e; HIPCHECK(hipEventCreate(&e)); c->tev[k].push_back(e); }
    HIPCHECK(hipEventRecord(c->tev[k][c->tev_used[k]++], st));
    return 0;
}

static void dec_free(DecCtx *c) {
    if (!c) return;
    (void)dec_sync_all(c);
    dec_streamed_release(c);
    for (auto *v : {&c->ev_hdr, &c->ev_parsed, &c->ev_recon})
        for (auto e : *v) if (e) (void)hipEventDestroy(e);
    if (c->ev_in) (void)hipEventDestroy(c->ev_in);
    for (int k = 0; k < 2; k++) for (auto e : c->tev[k]) (void)hipEventDestroy(e);
    for (int i = 0; i < DecCtx::PMAX; i++) if (c->pst[i]) (void)hipStreamDestroy(c->pst[i]);
    (void)hipFree(c->d_pool);
    (void)hipFree(c->d_conc);
    if (c->h_in) (void)hipHostFree(c->h_in);
    (void)hipFree(c->d_nal);
    (void)hipFree(c->d_rgba);
    (void)hipFree(c->d_tight);
    (void)hipFree(c->d_prof);
    (void)hipFree(c->d_rprof);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// HBM layout per stream: cur | pic0 | pic1 | granules | deblock granules, then per frame slot:
// MbInfo[nmb] | MbCoef[nmb] | DecFrame. Everything is allocated once, in one pool. The ring holds
// NG groups of B slots. ng <= 0 picks enough groups that the parse of a call rarely waits for the
// reconstruction of the call that last used its slots (up to 16, fewer for large B) -- what a pipelined
// batch caller wants; a caller that synchronises on every call (the C-ABI decoder) passes ng = 2 and
// np = 1 (nothing would overlap: 8 MB per 1080p slot instead of 16 slots' worth).
static DecCtx *dec_create(int mbw, int mbh, int S, hipStream_t stream, int B = 1, int ng = 0, int np = DEC_PSTREAMS) {
    if (mbw <= 0 || mbh <= 0 || mbw > H264MI_MAX_MBS || mbh > H264MI_MAX_MBS || S <= 0 || B <= 0 ||
        S > H264MI_MAX_STREAMS || S * B > 4096 || ng > 16 || np < 1 || np > DecCtx::PMAX) return nullptr;
    wait_limit_from_env();
    DecCtx *c = new DecCtx();
    c->mbw = mbw; c->mbh = mbh; c->nmb = mbw * mbh; c->cw = mbw * 16; c->ch = mbh * 16; c->S = S; c->B = B;
    c->NG = ng > 0 ? std::max(2, ng) : std::max(2, std::min(16, 32 / B));
    c->np = np;
    if (stream) { c->stream = stream; c->own_stream = false; }
    else { if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return nullptr; } c->own_stream = true; }
    const size_t ysz = (size_t)c->cw * c->ch, csz = ysz / 4, pic = ysz + 2 * csz;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t off_p0 = al(pic), off_p1 = off_p0 + al(pic), off_gran = off_p1 + al(pic);
    const size_t off_dgran = off_gran + al(8 * (size_t)H264MI_GRANULES_PER_MB * c->nmb);
    const size_t off_egr = off_dgran + al(8 * (size_t)H264MI_DBK_GRANULES_PER_MB * c->nmb);
    const size_t lps = (size_t)c->cw + 2 * H264MI_LPADX, lph = (size_t)c->ch + 2 * H264MI_LPADY;
    const size_t cps = (size_t)c->cw / 2 + 2 * H264MI_CPADX, cph = (size_t)c->ch / 2 + 2 * H264MI_CPADY;
    // reference planes: the padded integer luma plane and padded chroma (no half-sample planes: dec_recon.inc
    // interpolates from the integer plane -- 3 x 2.3 MB per 1080p stream less than the encoder's layout)
    const size_t off_pl = off_egr + al(8 * 128 * (size_t)c->nmb), off_plc = off_pl + al(lps * lph);
    const size_t per_stream = off_plc + 2 * al(cps * cph);
    const size_t off_coef = al(sizeof(MbInfo) * c->nmb), off_frm = off_coef + al(sizeof(MbCoef) * c->nmb);
    const size_t off_rgr = off_frm + al(sizeof(DecFrame));
    const size_t per_slot = off_rgr + al(8 * (size_t)H264MI_RES_GRANULES_PER_MB * c->nmb);
    const int NS = c->NG * B;  // frame slots: NG groups of B
    const size_t nsl = (size_t)S * NS;
    const size_t hdr = al(sizeof(DecState) * S) + al(sizeof(PlanesDesc) * S) + al(sizeof(DecDesc) * nsl) + al(sizeof(DbkDesc) * nsl) +
                       al(sizeof(DecInput) * nsl) + al(sizeof(uint32_t) * 2 * NS) + al(sizeof(uint32_t) * 16);
    const size_t total = hdr + per_stream * S + per_slot * nsl;
    if (hipMalloc(&c->d_pool, total) != hipSuccess) { if (c->own_stream) (void)hipStreamDestroy(c->stream); delete c; return nullptr; }
    c->pool_bytes = total;
    (void)hipMemsetAsync(c->d_pool, 0, total, c->stream);
    uint8_t *p = c->d_pool;
    c->d_st = (DecState *)p; p += al(sizeof(DecState) * S);
    c->d_pd = (PlanesDesc *)p; p += al(sizeof(PlanesDesc) * S);
    c->d_desc = (DecDesc *)p; p += al(sizeof(DecDesc) * nsl);
    c->d_dbk = (DbkDesc *)p; p += al(sizeof(DbkDesc) * nsl);
    c->d_in = (DecInput *)p; p += al(sizeof(DecInput) * nsl);
    c->d_ticket = (uint32_t *)p; p += al(sizeof(uint32_t) * 2 * NS);
    c->d_rticket = (uint32_t *)p; p += al(sizeof(uint32_t) * 16);
    uint8_t *streams = p, *slots = p + per_stream * S;
    c->h_desc.resize(nsl);
    if (hipHostMalloc((void **)&c->h_in, sizeof(DecInput) * nsl, hipHostMallocDefault) != hipSuccess) c->h_in = nullptr;
    std::vector<DbkDesc> hd(nsl);
    std::vector<PlanesDesc> hp(S);
    for (int f = 0; f < NS; f++)
        for (int s = 0; s < S; s++) {
            uint8_t *b = streams + per_stream * s, *q = slots + per_slot * ((size_t)f * S + s);
            DecDesc &d = c->h_desc[(size_t)f * S + s];
            uint8_t *cur = b, *p0 = b + off_p0, *p1 = b + off_p1;
            d.cur[0] = cur; d.cur[1] = cur + ysz; d.cur[2] = cur + ysz + csz;
            d.pic[0][0] = p0; d.pic[0][1] = p0 + ysz; d.pic[0][2] = p0 + ysz + csz;
            d.pic[1][0] = p1; d.pic[1][1] = p1 + ysz; d.pic[1][2] = p1 + ysz + csz;
            d.gran = (uint64_t *)(b + off_gran); d.dgran = (uint64_t *)(b + off_dgran);
            d.info = (MbInfo *)q; d.coef = (MbCoef *)(q + off_coef); d.frm = (DecFrame *)(q + off_frm);
            d.st = c->d_st + s; d.cw = c->cw; d.ch = c->ch; d.egran = (uint64_t *)(b + off_egr);
            d.rgran = (uint64_t *)(q + off_rgr);
            d.pl = b + off_pl + H264MI_LPADY * lps + H264MI_LPADX;
            for (int k = 0; k < 2; k++) d.plc[k] = b + off_plc + k * al(cps * cph) + H264MI_CPADY * cps + H264MI_CPADX;
            d.ps = (int)lps; d.psc = (int)cps;
            if (f == 0) {  // planes of the stream's reference picture, built after each reconstructed frame
                PlanesDesc &pd = hp[s];
                for (int i = 0; i < 3; i++) { pd.src[0][i] = d.pic[0][i]; pd.src[1][i] = d.pic[1][i]; }
                pd.parity = &c->d_st[s].parity; pd.active = &c->d_st[s].got_pic;
                pd.pl[0] = d.pl; pd.pl[1] = pd.pl[2] = pd.pl[3] = nullptr;  // dec_planes_kernel writes G and chroma only
                pd.plc[0] = d.plc[0]; pd.plc[1] = d.plc[1]; pd.ps = d.ps; pd.psc = d.psc;
            }
            DbkDesc &k = hd[(size_t)f * S + s];
            for (int i = 0; i < 3; i++) { k.rec[i] = d.cur[i]; k.out[0][i] = d.pic[1][i]; k.out[1][i] = d.pic[0][i]; }
            k.info = d.info; k.dgran = d.dgran; k.epoch = &c->d_st[s].epoch; k.disable = nullptr;  // per MB (slice word)
            k.active = &c->d_st[s].got_pic; k.parity = &c->d_st[s].parity; k.abort_word = &c->d_st[s].err; k.src_gran = d.egran;
        }
    (void)hipMemcpyAsync(c->d_desc, c->h_desc.data(), sizeof(DecDesc) * nsl, hipMemcpyHostToDevice, c->stream);
    (void)hipMemcpyAsync(c->d_dbk, hd.data(), sizeof(DbkDesc) * nsl, hipMemcpyHostToDevice, c->stream);
    (void)hipMemcpyAsync(c->d_pd, hp.data(), sizeof(PlanesDesc) * S, hipMemcpyHostToDevice, c->stream);
    if (hipMalloc(&c->d_conc, sizeof(int32_t) * (size_t)S * B) != hipSuccess) c->d_conc = nullptr;
    else (void)hipMemsetAsync(c->d_conc, 0, sizeof(int32_t) * (size_t)S * B, c->stream);
    if (getenv("H264MI_RECON_PROF") && hipMalloc(&c->d_rprof, sizeof(uint64_t) * 16) == hipSuccess)
        (void)hipMemsetAsync(c->d_rprof, 0, sizeof(uint64_t) * 16, c->stream);
    if (getenv("H264MI_PARSE_PROF") && hipMalloc(&c->d_prof, sizeof(uint64_t) * 16 * nsl) == hipSuccess)
        (void)hipMemsetAsync(c->d_prof, 0, sizeof(uint64_t) * 16 * nsl, c->stream);
    c->lds_bytes = RING_BYTES + 2 * 4 * (size_t)mbw;  // RBSP ring + per column {luma, chroma} TotalCoeff contexts
    c->lds_min = c->lds_bytes;
    bool ok = c->h_in && c->d_conc && hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < c->np && ok; i++) ok = hipStreamCreateWithFlags(&c->pst[i], hipStreamNonBlocking) == hipSuccess;
    for (auto *v : {&c->ev_hdr, &c->ev_parsed, &c->ev_recon}) {
        v->assign(c->NG, nullptr);
        for (int g = 0; g < c->NG && ok; g++) ok = hipEventCreateWithFlags(&(*v)[g], hipEventDisableTiming) == hipSuccess;
    }
    // every group starts free and the header chain starts settled
    for (int g = 0; g < c->NG && ok; g++) ok = hipEventRecord(c->ev_recon[g], c->stream) == hipSuccess && hipEventRecord(c->ev_hdr[g], c->stream) == hipSuccess;
    const int lds_cap = (int)std::max(c->lds_bytes, (size_t)40 * 1024);  // room for the reserved-lane padding
    if (!ok || hipFuncSetAttribute((const void *)dec_parse_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_cap) != hipSuccess ||
        hipFuncSetAttribute((const void *)dec_parse_prof_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_cap) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        dec_free(c);
        return nullptr;
    }
    dec_set_streamed(c, getenv("H264MI_DEC_STREAMED") ? atoi(getenv("H264MI_DEC_STREAMED")) : -1);
    if (const char *e = getenv("H264MI_DEC_RESOLVE")) c->resolve = atoi(e) != 0;
    return c;
}

// Decode n access units per stream (n <= B): in[f * S + s] is frame f of stream s. The call takes
// the next group of B frame slots. On one of two parse streams (alternating by call): wait until the
// reconstruction that last used the group is done, the inputs are ready and the previous call's
// header pass has committed its parameter sets; then NAL scan, headers (all n x S frames at once),
// and slice data (all n x S slices at once). The reconstruction stream then reconstructs and
// deblocks the frames in order. Two calls' slice data are thus entropy-decoded concurrently while
// earlier calls reconstruct.
// Input ordering: the NAL bytes and device sizes are read on the parse stream. With ready == null
// the parse waits for everything enqueued on the decoder's stream before this call (stream order);
// with events, it waits only for those (the producer's).
static int dec_frames(DecCtx *c, int n, const DecInput *in, const hipEvent_t *ready = nullptr, int nready = 0) {
    // the reconstruction gate (h264mi_dec_set_recon_gate) applies to this call only, whether it succeeds or
    // returns -1 part-way: taken into locals and cleared before anything can fail (ADVICE r5)
    const uint32_t *rg_counter = c->rg_counter;
    const uint32_t rg_target = c->rg_target, rg_step = c->rg_step, rg_limit = c->rg_limit;
    const int rg_count = c->rg_count;
    c->rg_counter = nullptr;
    if (n <= 0 || n > c->B) return -1;
    const int S = c->S, ns = n * S, g = c->grp, slot0 = g * c->B;
    const uint32_t pin = c->calls & 1, tag = c->calls + 1;
    const int conceal = c->conceal;
    const int streamed = conceal ? 0 : c->streamed;  // gaps are known only once every slice of the picture is parsed
    // a streamed call reconstructs while its slice data is still being parsed: nothing can resolve ahead of it
    const int pre = streamed ? 0 : c->resolve;
    hipStream_t ps = c->pst[c->calls % c->np];
    DecDesc *dd = c->d_desc + (size_t)slot0 * S;
    HIPCHECK(hipStreamWaitEvent(ps, c->ev_recon[g], 0));
    if (nready <= 0) { HIPCHECK(hipEventRecord(c->ev_in, c->stream)); ready = &c->ev_in; nready = 1; }
    for (int i = 0; i < nready; i++) HIPCHECK(hipStreamWaitEvent(ps, ready[i], 0));
    HIPCHECK(hipStreamWaitEvent(ps, c->ev_hdr[(g + c->NG - 1) % c->NG], 0));  // header chain
    // the group's pinned input entries are free once the header pass of its previous call ran (that
    // is after its copy); NG calls ago, so this normally does not wait
    HIPCHECK(hipEventSynchronize(c->ev_hdr[g]));
    bool outputs = false;
    for (int i = 0; i < ns; i++) { c->h_in[(size_t)slot0 * S + i] = in[i]; outputs = outputs || in[i].out || in[i].got; }
    HIPCHECK(hipMemcpyAsync(c->d_in + (size_t)slot0 * S, c->h_in + (size_t)slot0 * S, sizeof(DecInput) * ns,
                            hipMemcpyHostToDevice, ps));
    hipLaunchKernelGGL(dec_scan_kernel, dim3(ns), dim3(64), 0, ps, DecScanLaunch{S, n, c->d_in + (size_t)slot0 * S, dd});
    hipLaunchKernelGGL(dec_hdr_kernel, dim3(ns), dim3(64), 0, ps, DecParseLaunch{S, n, c->mbw, c->mbh, (int)pin, dd, nullptr, 1, tag, streamed});
    HIPCHECK(hipEventRecord(c->ev_hdr[g], ps));
    if (dec_time_mark(c, 1, ps)) return -1;
    hipLaunchKernelGGL(c->d_prof ? dec_parse_prof_kernel : dec_parse_kernel, dim3(ns * c->slice_waves), dim3(64), c->lds_bytes, ps,
                       DecParseLaunch{S, n, c->mbw, c->mbh, (int)pin, dd, c->d_prof ? c->d_prof + (size_t)slot0 * S * 16 : nullptr,
                                      c->slice_waves, tag, streamed});
    if (conceal)  // the gap records of every picture of the call (they depend on no sample: one launch serves all frames;
                  // what does depend on the frame before -- is there a reference -- is dec_frame_begin_kernel's, per frame)
        hipLaunchKernelGGL(dec_conceal_kernel, dim3(ns, (c->nmb + CONCEAL_SPAN - 1) / CONCEAL_SPAN), dim3(256), 0, ps,
                           DecConcealLaunch{ns, c->mbw, c->mbh, dd});
    if (pre) {  // every picture of the call, before ev_parsed
        hipLaunchKernelGGL(dec_resolve_kernel, dim3(ns * c->mbh), dim3(64), 0, ps,
                           DecResolveLaunch{ns, c->mbw, c->mbh, dd, c->d_rticket + g, c->rt_base[g], tag, conceal});
        c->rt_base[g] += (uint32_t)(ns * c->mbh);
        c->resolve_launches++;
    }
    if (dec_time_mark(c, 1, ps)) return -1;
    HIPCHECK(hipEventRecord(c->ev_parsed[g], ps));
    // --- reconstruction (decoder stream), frames in order. Streamed: frame 0 starts once the headers are
    // parsed and follows its slice data row by row (dec_frame_check_kernel then confirms the picture); the
    // later frames of the call, and every frame otherwise, start once the call's slice data is parsed.
    HIPCHECK(hipStreamWaitEvent(c->stream, streamed ? c->ev_hdr[g] : c->ev_parsed[g], 0));
    for (int f = 0; f < n; f++) {
        const DecDesc *df = dd + (size_t)f * S;
        hipLaunchKernelGGL(dec_frame_begin_kernel, dim3((S + 63) / 64), dim3(64), 0, c->stream,
                           DecBeginLaunch{S, f, dd, streamed, c->d_ticket + 2 * (slot0 + f), conceal, c->d_conc});
        if (streamed && f == 0 && c->gate_rows > 0)  // a forced (large) streamed launch follows the parse's last quarter only
            hipLaunchKernelGGL(dec_gate_kernel, dim3(1), dim3(64), 0, c->stream, DecGateLaunch{S, df, tag, (uint32_t)c->gate_rows});
        if (rg_counter && f < rg_count)
            hipLaunchKernelGGL(dec_wait_counter_kernel, dim3(1), dim3(64), 0, c->stream,
                               DecWaitLaunch{rg_counter, rg_target + (uint32_t)f * rg_step, rg_limit});
        // reconstruction rows and the deblocking rows that trail them, one launch
        if (dec_time_mark(c, 0, c->stream)) return -1;
        hipLaunchKernelGGL(pre ? dec_recon_pre_kernel : dec_recon_kernel, dim3(2 * S * c->mbh), dim3(64), 0, c->stream,
                           DecLaunch{S, c->mbw, c->mbh, df, c->d_ticket + 2 * (slot0 + f), c->d_dbk + (size_t)(slot0 + f) * S, c->d_rprof,
                                     tag, streamed});
        if (dec_time_mark(c, 0, c->stream)) return -1;
        if (streamed && f == 0) HIPCHECK(hipStreamWaitEvent(c->stream, c->ev_parsed[g], 0));
        hipLaunchKernelGGL(dec_end_kernel, dim3((S + 63) / 64), dim3(64), 0, c->stream, DecEndLaunch{S, df, streamed});
        if (outputs && in[0].fmt == H264MI_FMT_LAYOUT) {  // the layout in force travels by value in the launch
            if (launch_dec_output_layout(S, c->cw, c->ch, c->w, c->h, df, c->d_in + (size_t)(slot0 + f) * S, c->out_lay, c->stream) != 0) return -1;
        } else if (outputs && in[0].fmt == H264MI_FMT_RGBA && !colorspec_default(c->out_cs)) {  // likewise the specification in force
            if (launch_dec_output_rgba_cs(S, c->cw, c->ch, df, c->d_in + (size_t)(slot0 + f) * S, c->out_cs, c->stream) != 0) return -1;
        } else if (outputs && in[0].fmt == H264MI_FMT_RGBA) {  // every frame's picture to the caller (DecInput::out / got)
            const dim3 cg = color_grid(c->cw, c->ch, S);
            hipLaunchKernelGGL(dec_output_rgba_kernel, dim3(cg.x, S), dim3(256), 0, c->stream,
                               DecOutLaunch{S, c->cw, c->ch, df, c->d_in + (size_t)(slot0 + f) * S});
        } else if (outputs)
            hipLaunchKernelGGL(dec_output_kernel, dim3((2 * c->ch + 3) / 4, S), dim3(256), 0, c->stream,
                               DecOutLaunch{S, c->cw, c->ch, df, c->d_in + (size_t)(slot0 + f) * S});
        if (launch_dec_planes(S, c->cw, c->ch, c->d_pd, c->stream) != 0) return -1;  // the next frame's padded reference planes
    }
    HIPCHECK(hipEventRecord(c->ev_recon[g], c->stream));
    HIPCHECK(hipGetLastError());
    c->grp = (g + 1) % c->NG;
    c->calls++;
    c->last_n = n;
    return 0;
}
// Parse streams: each decode call's entropy decoding runs on the next of np streams, so up to np calls
// entropy-decode concurrently (bounded by the NG slot groups). More streams suit callers that decode
// one frame per call while frames keep arriving (each stream wants its own hardware queue).
// A CU mask over bits [lo, hi) of the device's CUs (complement: every other CU). The runtime stripes
// mask bits over the XCDs (tools/micro/cu_probe.hip: bits [0, 16) = two CUs on each of the 8 XCDs).
static std::vector<uint32_t> cu_mask(int lo, int hi, bool complement) {
    int ncu = 0, dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0)
        ncu = 256;
    std::vector<uint32_t> m((size_t)(ncu + 31) / 32, 0);
    for (int i = 0; i < ncu; i++)
        if ((i >= lo && i < hi) != complement) m[(size_t)i / 32] |= 1u << (i % 32);
    return m;
}
// Entropy decoding on reserved CUs: the parse streams are recreated with a CU mask of bits [lo, hi).
// The slice chains are long and few; on CUs shared with the wavefront kernels of an encoder or of
// the reconstruction, each decode call's NAL scan, header and slice-data launches wait for free
// workgroup slots (measured: up to one encoder frame each). Callers keep their own wavefront streams
// off these CUs (h264mi_stream_create_cus(lo, hi, 1)). lo == hi: no mask.
static int dec_set_parse_cus(DecCtx *c, int lo, int hi) {
    if (lo < 0 || hi < lo) return -1;
    if (dec_sync_all(c) != hipSuccess) return -1;
    const std::vector<uint32_t> m = cu_mask(lo, hi, false);
    c->cu_lo = lo; c->cu_hi = hi;
    // On the reserved CUs each slice wave asks for a quarter of the CU's 160 KB of LDS: at most four
    // slice waves per CU, which the dispatcher spreads over its four SIMDs -- a serial chain never
    // shares a SIMD's issue slots with another one (two chains on one SIMD each run at about half speed).
    c->lds_bytes = lo == hi ? c->lds_min : std::max(c->lds_min, (size_t)40 * 1024);
    for (int i = 0; i < DecCtx::PMAX; i++) {
        if (!c->pst[i]) continue;
        if (hipStreamDestroy(c->pst[i]) != hipSuccess) return -1;
        c->pst[i] = nullptr;
        const hipError_t e = lo == hi ? hipStreamCreateWithFlags(&c->pst[i], hipStreamNonBlocking)
                                      : hipExtStreamCreateWithCUMask(&c->pst[i], (uint32_t)m.size(), m.data());
        if (e != hipSuccess) return -1;
    }
    return 0;
}
static int dec_set_parse_streams(DecCtx *c, int n) {
    if (n < 1 || n > DecCtx::PMAX) return -1;
    if (dec_sync_all(c) != hipSuccess) return -1;
    const std::vector<uint32_t> m = cu_mask(c->cu_lo, c->cu_hi, false);
    for (int i = c->np; i < n; i++) {
        if (c->pst[i]) continue;
        const hipError_t e = c->cu_lo == c->cu_hi ? hipStreamCreateWithFlags(&c->pst[i], hipStreamNonBlocking)
                                                  : hipExtStreamCreateWithCUMask(&c->pst[i], (uint32_t)m.size(), m.data());
        if (e != hipSuccess) return -1;
    }
    c->np = n;
    return 0;
}
static int dec_frame(DecCtx *c, const uint8_t *const *d_nal, const int *nbytes, const int32_t *const *nbytes_dev = nullptr,
                     uint8_t *const *d_out = nullptr) {
    std::vector<DecInput> in(c->S);
    for (int s = 0; s < c->S; s++) {
        in[s].nal = d_nal[s]; in[s].size = nbytes ? nbytes[s] : 0; in[s].size_dev = nbytes_dev ? nbytes_dev[s] : nullptr; in[s].fmt = H264MI_FMT_I420;
        in[s].out = d_out ? d_out[s] : nullptr; in[s].got = nullptr;
    }
    return dec_frames(c, 1, in.data());
}

// host_peek_sps (geometry of the first SPS, for the C-ABI decoder): host_sps.h

}  // namespace h264mi
