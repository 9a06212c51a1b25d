// capi_dec.inc -- extern "C" boundary, decoder half.
//   init_decoder :253-280, deinit_decoder :240-251, decode_frame_optimized :391-422,
//   decode_frame_yuv_i420 :424-464 (openh264_wrapper.cpp) with the same 32-slot pool semantics,
//   plus the device-resident batch decoder (h264mi_dec_*).
namespace h264mi {

// Decode one access unit held in host memory; returns 1 when a picture was produced, 2 when a
// damaged access unit was concealed by the last picture (which stays the reference), 0 when there
// is nothing to output. The wrapper outputs a picture only when DecodeFrameNoDelay returns 0
// (openh264_wrapper.cpp:407, :435); OpenH264 reports a concealed access unit with a non-zero
// dsDataErrorConcealed status, so the C-ABI below reports "no picture" (0 x 0) for rc 2.
static int dec_host_call(DecSlot *slot, const unsigned char *data, int size, DecState *st_out, bool tight = false) {
    int mbw = 0, mbh = 0;
    if (host_peek_sps(data, size, &mbw, &mbh) && (!slot->c || slot->c->mbw != mbw || slot->c->mbh != mbh)) {
        // one call in flight at a time (the call synchronises): two slot groups, one parse stream.
        // The working decoder is replaced only once its successor exists.
        DecCtx *n = dec_create(mbw, mbh, 1, nullptr, 1, 2, 1);
        if (n) n->slice_waves = 8;  // one picture per call: a multi-slice picture's slices parse concurrently
        // H264MI_DEC_CONCEAL=1: lost slices of a non-IDR picture are concealed by slice copy (DESIGN.md §6.5) and the
        // picture is returned; any other value, or none, leaves every access unit handled as before
        if (const char *e = getenv("H264MI_DEC_CONCEAL")) { if (n && !strcmp(e, "1")) n->conceal = 1; }
        if (!n) return 0;
        dec_free(slot->c);
        slot->c = n;
    }
    DecCtx *c = slot->c;
    if (!c) return 0;
    if (c->nal_cap < (size_t)size) {
        (void)hipFree(c->d_nal);
        c->d_nal = nullptr; c->nal_cap = 0;
        if (hipMalloc(&c->d_nal, size) != hipSuccess) return 0;
        c->nal_cap = size;
    }
    if (hipMemcpyAsync(c->d_nal, data, size, hipMemcpyHostToDevice, c->stream) != hipSuccess) return 0;
    const uint8_t *p = c->d_nal;
    if (tight && !c->d_tight) {
        if (hipMalloc(&c->d_tight, (size_t)c->cw * c->ch * 3 / 2) != hipSuccess) { c->d_tight = nullptr; return 0; }
        c->tight_cap = (size_t)c->cw * c->ch * 3 / 2;
    }
    uint8_t *out = tight ? c->d_tight : nullptr;  // the cropped picture, written on the device behind the frame
    if (dec_frame(c, &p, &size, nullptr, tight ? &out : nullptr) != 0) return 0;
    if (hipMemcpyAsync(st_out, c->d_st, sizeof(DecState), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return 0;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return 0;
    if (st_out->got_pic && !st_out->err) return 1;
    // ERROR_CON_FRAME_COPY (openh264_wrapper.cpp:269): a damaged access unit (parse error,
    // unsupported syntax, missing reference) is concealed by the last picture, which stays the
    // reference -- pic[parity] was not flipped, so the read-out below returns exactly that copy
    return st_out->err && st_out->has_ref ? 2 : 0;
}
}  // namespace h264mi

extern "C" {

void h264mi_i_deinit_decoder(h264mi_instance *I, int decoder_index) {
    if (!I || decoder_index < 0 || decoder_index >= MAX_DECODERS) return;
    if (I->decoder_pool[decoder_index]) {
        dec_free(I->decoder_pool[decoder_index]->c);
        delete I->decoder_pool[decoder_index];
        I->decoder_pool[decoder_index] = nullptr;
    }
}

int h264mi_i_init_decoder(h264mi_instance *I, int decoder_index) {
    if (!I || decoder_index < 0 || decoder_index >= MAX_DECODERS) return -1;
    h264mi_i_deinit_decoder(I, decoder_index);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        fprintf(stderr, "Failed to create decoder #%d\n", decoder_index);
        return -1;
    }
    I->decoder_pool[decoder_index] = new DecSlot{nullptr};
    printf("Successfully initialized decoder for stream %d\n", decoder_index);
    return 0;
}

void h264mi_i_decode_frame_yuv_i420_cap(h264mi_instance *I, int decoder_index, unsigned char *encoded_data, int size,
                                        unsigned char *out_yuv_buffer, size_t out_cap, int *out_width, int *out_height) {
    *out_width = 0; *out_height = 0;
    if (!I || decoder_index < 0 || decoder_index >= MAX_DECODERS || !I->decoder_pool[decoder_index]) return;
    if (!encoded_data || size <= 0) return;
    DecSlot *slot = I->decoder_pool[decoder_index];
    DecState st;
    if (dec_host_call(slot, encoded_data, size, &st, true) != 1) return;  // concealed (2) or nothing: no output
    DecCtx *c = slot->c;
    const int W = c->cw - 2 * (st.ps.crop[0] + st.ps.crop[1]), H = c->ch - 2 * (st.ps.crop[2] + st.ps.crop[3]);
    if ((size_t)W * H * 3 / 2 > out_cap) return;  // picture does not fit the caller's buffer
    // dec_output_kernel already wrote the cropped tight I420 picture to d_tight: one contiguous copy
    if (hipMemcpy(out_yuv_buffer, c->d_tight, (size_t)W * H * 3 / 2, hipMemcpyDeviceToHost) != hipSuccess) return;
    *out_width = W; *out_height = H;
}

void h264mi_i_decode_frame_optimized_cap(h264mi_instance *I, int decoder_index, unsigned char *encoded_data, int size,
                                         unsigned char *out_rgba_buffer, size_t out_cap, int *out_width, int *out_height) {
    *out_width = 0; *out_height = 0;
    if (!I || decoder_index < 0 || decoder_index >= MAX_DECODERS || !I->decoder_pool[decoder_index]) return;
    if (!encoded_data || size <= 0) return;
    DecSlot *slot = I->decoder_pool[decoder_index];
    DecState st;
    if (dec_host_call(slot, encoded_data, size, &st) != 1) return;  // concealed (2) or nothing: no output
    DecCtx *c = slot->c;
    const int W = c->cw - 2 * (st.ps.crop[0] + st.ps.crop[1]), H = c->ch - 2 * (st.ps.crop[2] + st.ps.crop[3]);
    const int x0 = 2 * st.ps.crop[0], y0 = 2 * st.ps.crop[2];
    const int par = st.outpar & 1;  // the picture just decoded (a non-reference one is not the reference)
    const DecDesc &d = c->h_desc[0];
    size_t n = (size_t)W * H * 4;
    if (n > out_cap) return;  // picture does not fit the caller's buffer
    if (c->rgba_cap < n) {
        (void)hipFree(c->d_rgba);
        c->d_rgba = nullptr; c->rgba_cap = 0;
        if (hipMalloc(&c->d_rgba, n) != hipSuccess) return;
        c->rgba_cap = n;
    }
    const I420Pics pics{d.pic[par][0] + (size_t)y0 * c->cw + x0, d.pic[par][1] + (size_t)(y0 / 2) * (c->cw / 2) + x0 / 2,
                        d.pic[par][2] + (size_t)(y0 / 2) * (c->cw / 2) + x0 / 2, 0, c->cw, c->cw / 2};
    if (W <= 0 || H <= 0 || launch_i420_to_rgba(pics, W, H, 1, c->d_rgba, c->stream) != 0) return;
    if (hipMemcpyAsync(out_rgba_buffer, c->d_rgba, n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return;
    *out_width = W; *out_height = H;
}

void h264mi_i_decode_frame_yuv_i420(h264mi_instance *I, int decoder_index, unsigned char *encoded_data, int size,
                                    unsigned char *out_yuv_buffer, int *out_width, int *out_height) {
    h264mi_i_decode_frame_yuv_i420_cap(I, decoder_index, encoded_data, size, out_yuv_buffer, SIZE_MAX, out_width, out_height);
}
void h264mi_i_decode_frame_optimized(h264mi_instance *I, int decoder_index, unsigned char *encoded_data, int size,
                                     unsigned char *out_rgba_buffer, int *out_width, int *out_height) {
    h264mi_i_decode_frame_optimized_cap(I, decoder_index, encoded_data, size, out_rgba_buffer, SIZE_MAX, out_width, out_height);
}
void *h264mi_host_alloc(size_t bytes) {
    void *p = nullptr;
    return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}
void h264mi_host_free(void *p) { if (p) (void)hipHostFree(p); }
void deinit_decoder(int decoder_index) { h264mi_i_deinit_decoder(&g_instance, decoder_index); }
int init_decoder(int decoder_index) { return h264mi_i_init_decoder(&g_instance, decoder_index); }
void decode_frame_yuv_i420(int decoder_index, unsigned char *encoded_data, int size, unsigned char *out_yuv_buffer,
                           int *out_width, int *out_height) {
    h264mi_i_decode_frame_yuv_i420(&g_instance, decoder_index, encoded_data, size, out_yuv_buffer, out_width, out_height);
}
void decode_frame_optimized(int decoder_index, unsigned char *encoded_data, int size, unsigned char *out_rgba_buffer,
                            int *out_width, int *out_height) {
    h264mi_i_decode_frame_optimized(&g_instance, decoder_index, encoded_data, size, out_rgba_buffer, out_width, out_height);
}

h264mi_instance *h264mi_instance_create(void) { return new h264mi_instance(); }
void h264mi_instance_destroy(h264mi_instance *I) {
    if (!I || I == &g_instance) return;
    for (int i = 0; i < MAX_DECODERS; i++) h264mi_i_deinit_decoder(I, i);
    if (I->encoder) enc_free(I->encoder);
    free(I->encoded_buffer);
    (void)hipFree(I->rgba_dev);
    delete I;
}

// ---------------------------------------------------------------- batch API
struct h264mi_decoder { DecCtx *c; };

h264mi_decoder *h264mi_dec_create(int width, int height, int nstreams, void *hip_stream) {
    return h264mi_dec_create_batch(width, height, nstreams, 1, hip_stream);
}
h264mi_decoder *h264mi_dec_create_batch(int width, int height, int nstreams, int max_frames, void *hip_stream) {
    return h264mi_dec_create_ring(width, height, nstreams, max_frames, 0, DEC_PSTREAMS, hip_stream);
}
h264mi_decoder *h264mi_dec_create_ring(int width, int height, int nstreams, int max_frames, int groups, int parse_streams,
                                       void *hip_stream) {
    if (width <= 0 || height <= 0 || groups < 0 || groups == 1) return nullptr;
    DecCtx *c = dec_create((width + 15) / 16, (height + 15) / 16, nstreams, (hipStream_t)hip_stream, max_frames, groups, parse_streams);
    if (c) { c->w = width; c->h = height; }
    return c ? new h264mi_decoder{c} : nullptr;
}
static size_t dec_bytes(const DecCtx *c) { return c ? c->pool_bytes + c->nal_cap + c->rgba_cap + c->tight_cap : 0; }
size_t h264mi_dec_device_bytes(h264mi_decoder *d) { return d ? dec_bytes(d->c) : 0; }
size_t h264mi_i_decoder_device_bytes(h264mi_instance *I, int decoder_index) {
    if (!I || decoder_index < 0 || decoder_index >= MAX_DECODERS || !I->decoder_pool[decoder_index]) return 0;
    return dec_bytes(I->decoder_pool[decoder_index]->c);
}
int h264mi_dec_decode_frames_out(h264mi_decoder *d, int nframes, const void *const *d_nal, const int *nal_bytes,
                                 const int *const *d_sizes, void *const *ready_events, int nevents, void *const *d_out,
                                 int *const *d_got) {
    if (!d || !d_nal || (!nal_bytes && !d_sizes) || nframes <= 0 || nframes > d->c->B || nevents < 0 ||
        (nevents > 0 && !ready_events)) return -1;
    std::vector<DecInput> in((size_t)nframes * d->c->S);
    const int fmt = d->c->out_lay_set ? H264MI_FMT_LAYOUT : d->c->out_fmt;
    for (size_t i = 0; i < in.size(); i++) {
        if (d_out && fmt == H264MI_FMT_RGBA && ((uintptr_t)d_out[i] & 3)) return -1;  // RGBA pixels are stored as dwords
        in[i].nal = (const uint8_t *)d_nal[i];
        in[i].size = nal_bytes ? nal_bytes[i] : 0;
        in[i].size_dev = d_sizes ? (const int32_t *)d_sizes[i] : nullptr;
        in[i].fmt = fmt;
        in[i].out = d_out ? (uint8_t *)d_out[i] : nullptr;
        in[i].got = d_got ? (int32_t *)d_got[i] : nullptr;
    }
    return dec_frames(d->c, nframes, in.data(), (const hipEvent_t *)ready_events, nevents);
}
int h264mi_dec_decode_frames_after_n(h264mi_decoder *d, int nframes, const void *const *d_nal, const int *nal_bytes,
                                     const int *const *d_sizes, void *const *ready_events, int nevents) {
    return h264mi_dec_decode_frames_out(d, nframes, d_nal, nal_bytes, d_sizes, ready_events, nevents, nullptr, nullptr);
}
int h264mi_dec_decode_frames_after(h264mi_decoder *d, int nframes, const void *const *d_nal, const int *nal_bytes,
                                   const int *const *d_sizes, void *ready_event) {
    return h264mi_dec_decode_frames_after_n(d, nframes, d_nal, nal_bytes, d_sizes, &ready_event, ready_event ? 1 : 0);
}
int h264mi_dec_decode_frames(h264mi_decoder *d, int nframes, const void *const *d_nal, const int *nal_bytes,
                             const int *const *d_sizes) {
    return h264mi_dec_decode_frames_after(d, nframes, d_nal, nal_bytes, d_sizes, nullptr);
}
int h264mi_dec_max_frames(h264mi_decoder *d) { return d ? d->c->B : 0; }
int h264mi_dec_ring_groups(h264mi_decoder *d) { return d ? d->c->NG : 0; }
int h264mi_dec_set_parse_streams(h264mi_decoder *d, int n) { return d ? dec_set_parse_streams(d->c, n) : -1; }
int h264mi_dec_set_slice_waves(h264mi_decoder *d, int k) {
    if (!d || k < 1 || k > H264MI_MAX_SLICES || dec_sync_all(d->c) != hipSuccess) return -1;
    d->c->slice_waves = k;
    return 0;
}
int h264mi_dec_set_streamed(h264mi_decoder *d, int mode) {
    if (!d) return -1;
    // each call captures its mode when it is enqueued (dec_frames), so a change needs no synchronisation --
    // except giving up an automatic share of the process's streaming budget, which in-flight launches of this
    // decoder may still be using
    if (d->c->streamed_auto && dec_sync_all(d->c) != hipSuccess) return -1;
    return dec_set_streamed(d->c, mode);
}
int h264mi_dec_streamed(h264mi_decoder *d) { return d && !d->c->conceal ? d->c->streamed : 0; }
int h264mi_dec_set_conceal(h264mi_decoder *d, int mode) {
    if (!d || mode < 0 || mode > 1) return -1;
    d->c->conceal = mode;  // each call captures it when it is enqueued (dec_frames)
    return 0;
}
int h264mi_dec_conceal(h264mi_decoder *d) { return d ? d->c->conceal : 0; }
int h264mi_dec_concealed(h264mi_decoder *d, int *mbs) {
    if (!d || !mbs) return -1;
    DecCtx *c = d->c;
    const int n = c->last_n;
    if (n > 0 && hipMemcpyAsync(mbs, c->d_conc, sizeof(int32_t) * (size_t)n * c->S, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return -1;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    return n;
}
const int *h264mi_dec_concealed_ptr(h264mi_decoder *d) { return d ? d->c->d_conc : nullptr; }
int h264mi_conceal_gaps(int total_mbs, int nsl, const int *first, const int *end, const int *ok, int *gaps, int max_gaps) {
    return conceal_gaps(total_mbs, nsl, first, end, ok, gaps, max_gaps);
}
int h264mi_dec_set_resolve(h264mi_decoder *d, int mode) {
    if (!d || mode < 0 || mode > 1) return -1;
    d->c->resolve = mode;  // each call captures it when it is enqueued (dec_frames)
    return 0;
}
long long h264mi_dec_resolve_launches(h264mi_decoder *d) { return d ? d->c->resolve_launches : -1; }
// what h264mi_dec_decode_frames_out writes to its d_out buffers; each call captures the format when it is
// enqueued (DecInput::fmt), so a change needs no synchronisation
int h264mi_dec_set_output_format(h264mi_decoder *d, int fmt) {
    if (!d || (fmt != H264MI_FMT_I420 && fmt != H264MI_FMT_RGBA)) return -1;
    d->c->out_fmt = fmt;
    d->c->out_lay_set = false;  // the last setter wins
    return 0;
}
int h264mi_dec_output_format(h264mi_decoder *d) { return d ? (d->c->out_lay_set ? H264MI_FMT_LAYOUT : d->c->out_fmt) : -1; }
// a layout instead of a format (DESIGN.md §5.10; pix_rows.h dec_output_rows_kernel), checked here against the size the
// decoder was created with; each call hands the layout in force to its read-out launches by value (dec_frames)
int h264mi_dec_set_output_layout(h264mi_decoder *d, const h264mi_pix_layout *layout) {
    if (!d) return -1;
    if (!layout) { d->c->out_lay_set = false; return 0; }
    if (!pix_layout_ok(layout, d->c->w, d->c->h)) return -1;
    d->c->out_lay = *layout;
    d->c->out_lay_set = true;
    return 0;
}
int h264mi_dec_output_layout(h264mi_decoder *d, h264mi_pix_layout *out) {
    if (!d) return -1;
    if (!d->c->out_lay_set) return 0;
    if (out) *out = d->c->out_lay;
    return 1;
}
// the specification of RGBA output (DESIGN.md §5.11; colorspace.hip dec_output_rgba_cs_kernel): kept whatever the format
// is; each call hands the one in force to its read-out launches by value (dec_frames)
int h264mi_dec_set_output_colorspec(h264mi_decoder *d, const h264mi_colorspec *spec) {
    if (!d || (spec && !colorspec_ok(spec))) return -1;
    d->c->out_cs = spec ? *spec : h264mi_colorspec{};
    return 0;
}
int h264mi_dec_output_colorspec(h264mi_decoder *d, h264mi_colorspec *out) {
    if (!d || !out) return -1;
    *out = d->c->out_cs;
    return 0;
}
int h264mi_dec_set_recon_gate(h264mi_decoder *d, const uint32_t *d_counter, uint32_t target, uint32_t step, int count, int limit_us) {
    if (!d || count < 0 || limit_us < 0 || limit_us > 1000000) return -1;
    DecCtx *c = d->c;
    c->rg_counter = count > 0 ? d_counter : nullptr;
    c->rg_target = target; c->rg_step = step; c->rg_count = count; c->rg_limit = (uint32_t)limit_us * 100u;
    return 0;
}
int h264mi_dec_set_streamed_budget(int waves) {
    g_streamed_budget.store(waves > 0 ? waves : 0);
    return dec_streamed_budget();
}
int h264mi_dec_set_parse_cus(h264mi_decoder *d, int cu_lo, int cu_hi) { return d ? dec_set_parse_cus(d->c, cu_lo, cu_hi) : -1; }
void *h264mi_stream_create_cus(int cu_lo, int cu_hi, int complement) {
    if (cu_lo < 0 || cu_hi < cu_lo) return nullptr;
    const std::vector<uint32_t> m = cu_mask(cu_lo, cu_hi, complement != 0);
    hipStream_t s = nullptr;
    return hipExtStreamCreateWithCUMask(&s, (uint32_t)m.size(), m.data()) == hipSuccess ? (void *)s : nullptr;
}
void h264mi_stream_destroy(void *hip_stream) { if (hip_stream) (void)hipStreamDestroy((hipStream_t)hip_stream); }
void h264mi_dec_destroy(h264mi_decoder *d) { if (d) { dec_free(d->c); delete d; } }
int h264mi_dec_decode(h264mi_decoder *d, const void *const *d_nal, const int *nal_bytes) {
    if (!d || !d_nal || !nal_bytes) return -1;
    return dec_frame(d->c, (const uint8_t *const *)d_nal, nal_bytes);
}
int h264mi_dec_decode_dev(h264mi_decoder *d, const void *const *d_nal, const int *const *d_sizes) {
    if (!d || !d_nal || !d_sizes) return -1;
    return dec_frame(d->c, (const uint8_t *const *)d_nal, nullptr, (const int32_t *const *)d_sizes);
}
int h264mi_dec_sync(h264mi_decoder *d) { return d && hipStreamSynchronize(d->c->stream) == hipSuccess ? 0 : -1; }
int h264mi_dec_status(h264mi_decoder *d, int *got_pic) {
    if (!d) return -1;
    std::vector<DecState> st(d->c->S);
    if (hipMemcpyAsync(st.data(), d->c->d_st, sizeof(DecState) * d->c->S, hipMemcpyDeviceToHost, d->c->stream) != hipSuccess) return -1;
    if (hipStreamSynchronize(d->c->stream) != hipSuccess) return -1;
    int err = 0;
    for (int s = 0; s < d->c->S; s++) { got_pic[s] = st[s].got_pic; err |= st[s].err; }
    return err ? -2 : 0;
}
const void *h264mi_dec_picture_ptr(h264mi_decoder *d, int stream) {
    if (!d || stream < 0 || stream >= d->c->S) return nullptr;
    DecState st;
    if (hipMemcpyAsync(&st, d->c->d_st + stream, sizeof(DecState), hipMemcpyDeviceToHost, d->c->stream) != hipSuccess) return nullptr;
    if (hipStreamSynchronize(d->c->stream) != hipSuccess) return nullptr;
    return d->c->h_desc[stream].pic[st.outpar & 1][0];
}
int h264mi_dec_set_timing(h264mi_decoder *d, int enable) {
    if (!d) return -1;
    DecCtx *c = d->c;
    if (dec_sync_all(c) != hipSuccess) return -1;
    c->timing = enable != 0;
    c->tev_used[0] = c->tev_used[1] = 0;
    return 0;
}
// total ms and launch count of dec_recon_kernel (which 0) or dec_parse_kernel (which 1) since
// set_timing (synchronises)
int h264mi_dec_kernel_time(h264mi_decoder *d, int which, double *ms_total, int *launches) {
    if (!d || which < 0 || which > 1) return -1;
    DecCtx *c = d->c;
    if (dec_sync_all(c) != hipSuccess) return -1;
    double t = 0;
    for (int i = 0; i + 1 < c->tev_used[which]; i += 2) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->tev[which][i], c->tev[which][i + 1]) != hipSuccess) return -1;
        t += ms;
    }
    *ms_total = t;
    *launches = c->tev_used[which] / 2;
    return 0;
}
int h264mi_dec_parse_profile(h264mi_decoder *d, uint64_t *out) {
    if (!d || !d->c->d_prof) return -1;
    // out: 16 per frame slot, h264mi_dec_ring_groups() x max_frames x nstreams slots
    return hipMemcpy(out, d->c->d_prof, sizeof(uint64_t) * 16 * d->c->S * d->c->B * d->c->NG, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
int h264mi_dec_coded_size(h264mi_decoder *d, int *cw, int *ch) {
    if (!d) return -1;
    *cw = d->c->cw; *ch = d->c->ch;
    return 0;
}
void *h264mi_dec_stream(h264mi_decoder *d) { return d ? (void *)d->c->stream : nullptr; }
int h264mi_dec_recon_profile(h264mi_decoder *d, uint64_t *out) {
    if (!d || !d->c->d_rprof) return -1;
    return hipMemcpy(out, d->c->d_rprof, sizeof(uint64_t) * 16, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
const char *h264mi_version(void) { return "h264mi 0.1 (gfx950)"; }

}  // extern "C"

// ---------------------------------------------------------------- colour conversion entry points
// Host-buffer wrappers of the edge conversions (rgba_to_yuv :22-40, yuv_to_rgba_optimized :150-195)
// for callers that hold frames in host memory; the device kernels are the same ones the encode /
// decode paths use.
extern "C" int h264mi_rgba_to_i420_host(const unsigned char *rgba, int w, int h, unsigned char *out_i420) {
    if (!rgba || !out_i420 || w <= 0 || h <= 0 || (w & 1) || (h & 1)) return -1;
    size_t n_in = (size_t)w * h * 4, n_out = (size_t)w * h * 3 / 2;
    uint8_t *d = nullptr;
    if (hipMalloc(&d, n_in + n_out) != hipSuccess) return -1;
    int rc = -1;
    if (hipMemcpy(d, rgba, n_in, hipMemcpyHostToDevice) == hipSuccess && launch_rgba_to_i420(d, w, h, 1, d + n_in, nullptr) == 0 &&
        hipMemcpy(out_i420, d + n_in, n_out, hipMemcpyDeviceToHost) == hipSuccess)
        rc = 0;
    (void)hipFree(d);
    return rc;
}
extern "C" int h264mi_i420_to_rgba_host(const unsigned char *i420, int w, int h, unsigned char *out_rgba) {
    if (!i420 || !out_rgba || w <= 0 || h <= 0 || (w & 1) || (h & 1)) return -1;
    size_t n_in = (size_t)w * h * 3 / 2, n_out = (size_t)w * h * 4;
    uint8_t *d = nullptr;
    if (hipMalloc(&d, n_in + n_out) != hipSuccess) return -1;
    int rc = -1;
    if (hipMemcpy(d, i420, n_in, hipMemcpyHostToDevice) == hipSuccess &&
        launch_i420_to_rgba(tight_i420(d, w, h), w, h, 1, d + n_in, nullptr) == 0 &&
        hipMemcpy(out_rgba, d + n_in, n_out, hipMemcpyDeviceToHost) == hipSuccess)
        rc = 0;
    (void)hipFree(d);
    return rc;
}
// Device-buffer forms: n tight frames back to back on both sides, one launch, asynchronous on the stream.
// The argument checks come before any HIP call.
extern "C" int h264mi_rgba_to_i420_dev(void *d_i420, const void *d_rgba, int w, int h, int n, void *hip_stream) {
    if (!d_i420 || !d_rgba || !color_args_ok(w, h, n) || ((uintptr_t)d_rgba & 3)) return -1;
    return launch_rgba_to_i420((const uint8_t *)d_rgba, w, h, n, (uint8_t *)d_i420, (hipStream_t)hip_stream);
}
extern "C" int h264mi_i420_to_rgba_dev(void *d_rgba, const void *d_i420, int w, int h, int n, void *hip_stream) {
    if (!d_rgba || !d_i420 || !color_args_ok(w, h, n) || ((uintptr_t)d_rgba & 3)) return -1;
    return launch_i420_to_rgba(tight_i420((const uint8_t *)d_i420, w, h), w, h, n, (uint8_t *)d_rgba, (hipStream_t)hip_stream);
}
