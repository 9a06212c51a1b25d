// capi_enc.inc -- extern "C" boundary, encoder half: the checks that belong to the boundary (null handle, null
// pointer, the arguments of the standalone *_dev calls) and forwards into the runtime (runtime_enc.inc; the stages in
// front of the frame step: enc_input.inc).
//
// (1) The reference wrapper surface (openh264_wrapper.cpp): init_encoder :198-228,
//     force_key_frame :230-236, encode_frame :315-356, encode_frame_yuv_i420 :358-389,
//     free_buffer :466-471 -- same signatures, same global-state and error semantics
//     (void functions report failure / skipped frames as *out_size = 0; init returns 0 / -1).
// (2) A device-resident batch API (h264mi_enc_*) for S independent streams of one geometry whose
//     frames are already in HBM -- the surface the benchmark and multi-GPU sharding drive.
#include "../../include/h264mi.h"

namespace h264mi {
#define MAX_DECODERS 32  // openh264_wrapper.cpp:8
struct DecSlot { DecCtx *c; };
}  // namespace h264mi

// The wrapper's global state (openh264_wrapper.cpp:11-18: encoder, decoder_pool[32], the grow-only
// encoded buffer and the RGBA->YUV scratch) as one instance. The plain entry points use a process-wide
// default instance (exactly the wrapper's globals); hosts that need the reference's one-state-per-
// wasm-instance semantics (a Worker per encoder / decoder set) create one instance each.
struct h264mi_instance {
    h264mi::EncCtx *encoder = nullptr;
    uint8_t *encoded_buffer = nullptr;
    int encoded_buffer_size = 0;
    uint8_t *rgba_dev = nullptr;
    size_t rgba_dev_size = 0;
    h264mi::DecSlot *decoder_pool[MAX_DECODERS] = {};
};

namespace h264mi {
static h264mi_instance g_instance;

// Read back one stream's frame after enc_frame(): returns bytes (0 on error)
static int enc_fetch(h264mi_instance *I, EncCtx *c, int s, uint8_t **out, int *out_size) {
    EncState st;
    if (hipMemcpyAsync(&st, c->d_st + s, sizeof(EncState), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return 0;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return 0;
    if (st.err || st.nal_bytes <= 0) return 0;
    if (I->encoded_buffer_size < st.nal_bytes) {
        free(I->encoded_buffer);
        I->encoded_buffer = (uint8_t *)malloc(st.nal_bytes);
        I->encoded_buffer_size = I->encoded_buffer ? st.nal_bytes : 0;
        if (!I->encoded_buffer) return 0;
    }
    const uint8_t *nal = c->h_desc[c->parity ^ 1][s].nal;  // the descriptor of the frame just coded
    if (hipMemcpy(I->encoded_buffer, nal, st.nal_bytes, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    *out = I->encoded_buffer;
    *out_size = st.nal_bytes;
    return st.nal_bytes;
}
}  // namespace h264mi

using namespace h264mi;

extern "C" {

int h264mi_i_init_encoder(h264mi_instance *I, int width, int height, int bitrate) {
    if (!I) return -1;
    if (I->encoder) { enc_free(I->encoder); I->encoder = nullptr; }
    I->encoder = enc_create(width, height, bitrate, 1, nullptr);
    return I->encoder ? 0 : -1;
}

void h264mi_i_force_key_frame(h264mi_instance *I) {
    if (I && I->encoder) {
        int one = 1;
        (void)hipMemcpyAsync(&I->encoder->d_st[0].force_idr, &one, sizeof(int), hipMemcpyHostToDevice, I->encoder->stream);
        (void)hipStreamSynchronize(I->encoder->stream);
        printf("Key frame forced.\n");
    }
}

void h264mi_i_encode_frame_yuv_i420(h264mi_instance *I, unsigned char *yuv, int width, int height, unsigned char **out_data,
                                    int *out_size) {
    *out_data = nullptr;
    *out_size = 0;
    EncCtx *c = I ? I->encoder : nullptr;
    if (!c || !yuv || width != c->w || height != c->h) return;
    if (hipMemcpyAsync(c->d_src, yuv, c->fbytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) return;
    if (enc_frame(c, c->d_src) != 0) return;
    enc_fetch(I, c, 0, out_data, out_size);
}

void h264mi_i_encode_frame(h264mi_instance *I, unsigned char *rgba, int width, int height, unsigned char **out_data, int *out_size) {
    *out_data = nullptr;
    *out_size = 0;
    EncCtx *c = I ? I->encoder : nullptr;
    if (!c || !rgba || width != c->w || height != c->h) return;
    size_t n = (size_t)width * height * 4;
    if (I->rgba_dev_size < n) {
        (void)hipFree(I->rgba_dev);
        I->rgba_dev = nullptr; I->rgba_dev_size = 0;
        if (hipMalloc(&I->rgba_dev, n) != hipSuccess) return;
        I->rgba_dev_size = n;
    }
    if (hipMemcpyAsync(I->rgba_dev, rgba, n, hipMemcpyHostToDevice, c->stream) != hipSuccess) return;
    if (launch_rgba_to_i420(I->rgba_dev, width, height, 1, c->d_src, c->stream) != 0) return;
    if (enc_frame(c, c->d_src) != 0) return;
    enc_fetch(I, c, 0, out_data, out_size);
}

int init_encoder(int width, int height, int bitrate) { return h264mi_i_init_encoder(&g_instance, width, height, bitrate); }
void force_key_frame(void) { h264mi_i_force_key_frame(&g_instance); }
void encode_frame_yuv_i420(unsigned char *yuv, int width, int height, unsigned char **out_data, int *out_size) {
    h264mi_i_encode_frame_yuv_i420(&g_instance, yuv, width, height, out_data, out_size);
}
void encode_frame(unsigned char *rgba, int width, int height, unsigned char **out_data, int *out_size) {
    h264mi_i_encode_frame(&g_instance, rgba, width, height, out_data, out_size);
}

void free_buffer(void *ptr) {
    if (ptr != nullptr) free(ptr);
}

// ---------------------------------------------------------------- batch API
struct h264mi_encoder { EncCtx *c; };

h264mi_encoder *h264mi_enc_create(int width, int height, int bitrate, int nstreams, void *hip_stream) {
    EncCtx *c = enc_create(width, height, bitrate, nstreams, (hipStream_t)hip_stream);
    if (!c) return nullptr;
    return new h264mi_encoder{c};
}
void h264mi_enc_destroy(h264mi_encoder *e) {
    if (!e) return;
    (void)hipStreamSynchronize(e->c->stream);
    enc_free(e->c);
    delete e;
}
int h264mi_enc_force_idr(h264mi_encoder *e, int stream) {
    if (!e) return -1;
    int one = 1;
    for (int s = 0; s < e->c->S; s++)
        if (stream < 0 || s == stream)
            if (hipMemcpyAsync(&e->c->d_st[s].force_idr, &one, sizeof(int), hipMemcpyHostToDevice, e->c->stream) != hipSuccess) return -1;
    return hipStreamSynchronize(e->c->stream) == hipSuccess ? 0 : -1;
}
// frame skipping by the rate control (DESIGN.md §3.6): on by default (the wrapper's OpenH264
// configuration); a skipped frame has nal_bytes 0 and leaves the reference unchanged
int h264mi_enc_set_frame_skip(h264mi_encoder *e, int enable) {
    if (!e) return -1;
    int v = enable != 0;
    for (int s = 0; s < e->c->S; s++)
        if (hipMemcpyAsync(&e->c->d_st[s].rc.skip_en, &v, sizeof(int), hipMemcpyHostToDevice, e->c->stream) != hipSuccess) return -1;
    return hipStreamSynchronize(e->c->stream) == hipSuccess ? 0 : -1;
}
// OpenH264's exact GOM rate control (DESIGN.md §3.6): each GOM's QP from the bits of every MB before it
int h264mi_enc_set_gom_exact(h264mi_encoder *e, int enable) {
    if (!e) return -1;
    if (enable && e->c->slices > 1) return -1;  // the rule restates OpenH264's single-slice budget (DESIGN.md §3.7)
    e->c->gom_exact = enable != 0;
    return 0;
}
// n slices of whole MB rows per picture from the next encode on (DESIGN.md §3.7). One host value for all streams:
// each frame step hands it to its begin kernel, which latches it per stream (enc_begin_stream) for the frame's other
// kernels, and picks the pack kernel by it -- frames already issued keep the count they were issued with
int h264mi_enc_set_slices(h264mi_encoder *e, int n) {
    if (!e || !slices_valid(e->c->mbh, n) || (n > 1 && e->c->gom_exact)) return -1;
    e->c->slices = n;
    return 0;
}
int h264mi_enc_slices(h264mi_encoder *e) { return e ? e->c->slices : -1; }
int h264mi_slice_first_row(int mbh, int n, int k) {
    if (mbh < 1 || !slices_valid(mbh, n) || k < 0 || k > n) return -1;
    return slice_first_row(mbh, n, k);
}
// Per-frame distortion records (DESIGN.md §5.2; runtime_enc.inc enc_set_quality)
int h264mi_enc_set_quality(h264mi_encoder *e, int enable) { return e ? enc_set_quality(e->c, enable != 0) : -1; }
int h264mi_enc_quality_enabled(h264mi_encoder *e) { return e ? (e->c->quality ? 1 : 0) : -1; }
int h264mi_enc_quality(h264mi_encoder *e, int stream, h264mi_quality *out) {
    if (!e || !out || !e->c->quality || stream < 0 || stream >= e->c->S) return -1;
    if (hipMemcpyAsync(out, e->c->d_qual + stream, sizeof(h264mi_quality), hipMemcpyDeviceToHost, e->c->stream) != hipSuccess) return -1;
    return hipStreamSynchronize(e->c->stream) == hipSuccess ? 0 : -1;
}
const h264mi_quality *h264mi_enc_quality_dev(h264mi_encoder *e) { return e && e->c->quality ? e->c->d_qual : nullptr; }
int h264mi_i420_quality_dev(h264mi_quality *d_out, const void *d_a, const void *d_b, int w, int h, int n, void *hip_stream) {
    if (!d_out || !d_a || !d_b || !quality_args_ok(w, h, n)) return -1;
    return launch_quality_i420(d_out, (const uint8_t *)d_a, (const uint8_t *)d_b, w, h, n, (hipStream_t)hip_stream);
}
double h264mi_psnr(uint64_t sse, uint64_t samples) {
    if (sse == 0) return 100.0;
    return 10.0 * log10(65025.0 * (double)samples / (double)sse);
}
int h264mi_enc_inject_error(h264mi_encoder *e, int stream, int code) {
    if (!e || stream < 0 || stream >= e->c->S || code <= 0) return -1;
    if (hipMemcpyAsync(&e->c->d_st[stream].inject_err, &code, sizeof(int), hipMemcpyHostToDevice, e->c->stream) != hipSuccess) return -1;
    return hipStreamSynchronize(e->c->stream) == hipSuccess ? 0 : -1;
}
int h264mi_enc_frames_skipped(h264mi_encoder *e, int stream) {
    if (!e || stream < 0 || stream >= e->c->S) return -1;
    EncState st;
    if (hipMemcpy(&st, e->c->d_st + stream, sizeof(EncState), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return st.skipped;
}
// The input chain (DESIGN.md §5.16; enc_input.inc): with a stage on the caller's frames are coded from the input area
int h264mi_enc_encode(h264mi_encoder *e, const void *d_frames) { return e && d_frames ? enc_encode(e->c, d_frames) : -1; }
int h264mi_enc_set_overlays(h264mi_encoder *e, const void *d_sprites, int ow, int oh, int nsprites, const h264mi_overlay *ov, int nov) {
    return e ? enc_set_overlays(e->c, d_sprites, ow, oh, nsprites, ov, nov) : -1;
}
int h264mi_enc_overlays(h264mi_encoder *e) { return e ? (int)e->c->in.ov.list.size() : -1; }
// The temporal denoiser (DESIGN.md §5.13; denoise.hip; the checks: picture_host.h): n frames, one launch
int h264mi_denoise_ok(const h264mi_denoise *p) { return denoise_ok(p) ? 0 : -1; }
int h264mi_i420_denoise_dev(void *d_dst, void *d_dst2, const void *d_cur, const void *d_prev, int w, int h, int n, const h264mi_denoise *p,
                            void *d_stats, void *hip_stream) {
    if (!denoise_args_ok(d_dst, d_dst2, d_cur, d_prev, w, h, n, p, d_stats)) return -1;
    return launch_denoise_i420((uint8_t *)d_dst, (uint8_t *)d_dst2, (const uint8_t *)d_cur, (const uint8_t *)d_prev, w, h, n, *p,
                               (uint32_t *)d_stats, (hipStream_t)hip_stream);
}
int h264mi_enc_set_denoise(h264mi_encoder *e, const h264mi_denoise *p) { return e ? enc_set_denoise(e->c, p) : -1; }
int h264mi_enc_denoise(h264mi_encoder *e, h264mi_denoise *out) { return e ? stage_get(e->c->in.dn, out) : -1; }
// The deinterlacer (DESIGN.md §5.15; deinterlace.hip; the checks: picture_host.h): n frames, one launch
int h264mi_deinterlace_ok(const h264mi_deinterlace *p) { return deinterlace_ok(p) ? 0 : -1; }
int h264mi_i420_deinterlace_dev(void *d_dst, void *d_prev_out, const void *d_cur, const void *d_prev, int w, int h, int n,
                                const h264mi_deinterlace *p, void *d_stats, void *hip_stream) {
    if (!deinterlace_args_ok(d_dst, d_prev_out, d_cur, d_prev, w, h, n, p, d_stats)) return -1;
    return launch_deinterlace_i420((uint8_t *)d_dst, (uint8_t *)d_prev_out, (const uint8_t *)d_cur, (const uint8_t *)d_prev, w, h, n, *p,
                                   (uint32_t *)d_stats, (hipStream_t)hip_stream);
}
int h264mi_i420_deinterlace_host(void *dst, const void *cur, const void *prev, int w, int h, const h264mi_deinterlace *p, uint32_t *stats) {
    if (!dst || !cur || !canvas_ok(w, h) || !deinterlace_ok(p)) return -1;
    deinterlace_frame_host((uint8_t *)dst, (const uint8_t *)cur, (const uint8_t *)prev, w, h, *p, stats);
    return 0;
}
int h264mi_enc_set_deinterlace(h264mi_encoder *e, const h264mi_deinterlace *p) { return e ? enc_set_deinterlace(e->c, p) : -1; }
int h264mi_enc_deinterlace(h264mi_encoder *e, h264mi_deinterlace *out) { return e ? stage_get(e->c->in.di, out) : -1; }
// The spatial filter and the privacy masks (DESIGN.md §5.18; spatial.hip; the checks: picture_host.h)
int h264mi_spatial_ok(const h264mi_spatial *p) { return spatial_ok(p) ? 0 : -1; }
int h264mi_i420_spatial_dev(void *d_dst, const void *d_src, int w, int h, int n, const h264mi_spatial *p, void *hip_stream) {
    if (!spatial_args_ok(d_dst, d_src, w, h, n, p)) return -1;
    return launch_spatial_i420((uint8_t *)d_dst, (const uint8_t *)d_src, w, h, n, *p, (hipStream_t)hip_stream);
}
int h264mi_i420_spatial_host(void *dst, const void *src, int w, int h, const h264mi_spatial *p) {
    if (!spatial_args_ok(dst, src, w, h, 1, p)) return -1;
    spatial_frame_host((uint8_t *)dst, (const uint8_t *)src, w, h, *p);
    return 0;
}
int h264mi_privacy_ok(const h264mi_privacy *list, int n, int w, int h, int nframes) { return privacy_ok(list, n, w, h, nframes) ? 0 : -1; }
int h264mi_i420_privacy_dev(void *d_frames, int w, int h, int nframes, const h264mi_privacy *list, int nlist, void *hip_stream) {
    if (!d_frames || !privacy_ok(list, nlist, w, h, nframes)) return -1;
    return launch_privacy_i420((uint8_t *)d_frames, w, h, list, nlist, (hipStream_t)hip_stream);
}
int h264mi_i420_privacy_host(void *frames, int w, int h, int nframes, const h264mi_privacy *list, int nlist) {
    if (!frames || !privacy_ok(list, nlist, w, h, nframes)) return -1;
    privacy_frames_host((uint8_t *)frames, w, h, list, nlist);
    return 0;
}
int h264mi_enc_set_spatial(h264mi_encoder *e, const h264mi_spatial *p) { return e ? enc_set_spatial(e->c, p) : -1; }
int h264mi_enc_spatial(h264mi_encoder *e, h264mi_spatial *out) { return e ? stage_get(e->c->in.sp, out) : -1; }
int h264mi_enc_set_privacy(h264mi_encoder *e, const h264mi_privacy *list, int n) { return e ? enc_set_privacy(e->c, list, n) : -1; }
int h264mi_enc_privacy(h264mi_encoder *e) { return e ? (int)e->c->in.pv.list.size() : -1; }
// Histograms, level tables and automatic levels (DESIGN.md §5.19; levels.hip; the checks: picture_host.h)
int h264mi_levels_ok(const h264mi_levels *p) { return levels_ok(p) ? 0 : -1; }
int h264mi_i420_hist_dev(void *d_hist, const void *d_frames, int w, int h, int n, void *hip_stream) {
    if (!hist_args_ok(d_hist, d_frames, w, h, n)) return -1;
    return launch_hist_i420((uint32_t *)d_hist, (const uint8_t *)d_frames, w, h, n, (hipStream_t)hip_stream);
}
int h264mi_i420_lut_dev(void *d_dst, const void *d_src, int w, int h, int n, const void *d_luts, int per_frame, void *hip_stream) {
    if (!lut_args_ok(d_dst, d_src, w, h, n, d_luts, per_frame)) return -1;
    return launch_lut_i420((uint8_t *)d_dst, (const uint8_t *)d_src, w, h, n, (const uint8_t *)d_luts, per_frame, (hipStream_t)hip_stream);
}
size_t h264mi_levels_work_bytes(int n) { return n < 1 ? 0 : levels_work_bytes(n); }
int h264mi_i420_levels_dev(void *d_dst, const void *d_src, int w, int h, int n, const h264mi_levels *p, void *d_state, void *d_record,
                           void *d_work, void *hip_stream) {
    if (!levels_args_ok(d_dst, d_src, w, h, n, p, d_state, d_record, d_work)) return -1;
    return launch_levels_i420((uint8_t *)d_dst, (const uint8_t *)d_src, w, h, n, *p, (int32_t *)d_state, (int32_t *)d_record, (uint8_t *)d_work,
                              (hipStream_t)hip_stream);
}
int h264mi_i420_hist_host(uint32_t *hist, const void *frame, int w, int h) {
    if (!hist || !frame || !canvas_ok(w, h)) return -1;
    hist_frame_host(hist, (const uint8_t *)frame, w, h);
    return 0;
}
int h264mi_i420_lut_host(void *dst, const void *src, int w, int h, const uint8_t *lut768) {
    if (!dst || !src || !lut768 || !canvas_ok(w, h)) return -1;
    lut_frame_host((uint8_t *)dst, (const uint8_t *)src, w, h, lut768);
    return 0;
}
int h264mi_levels_lut_host(uint8_t *lut768, const uint32_t *hist_y, int w, int h, const h264mi_levels *p, int32_t *state4, int32_t *record8) {
    if (!lut768 || !canvas_ok(w, h) || !levels_ok(p) || (p->mode == H264MI_LEVELS_AUTO && !hist_y)) return -1;
    levels_lut_host(lut768, hist_y, w, h, *p, state4, record8);
    return 0;
}
int h264mi_enc_set_levels(h264mi_encoder *e, const h264mi_levels *p) { return e ? enc_set_levels(e->c, p) : -1; }
int h264mi_enc_levels(h264mi_encoder *e, h264mi_levels *out) { return e ? stage_get(e->c->in.lv, out) : -1; }
int h264mi_enc_levels_record(h264mi_encoder *e, int32_t *out, int nstreams) {
    if (!e || !out || !e->c->in.lv.on || nstreams != e->c->S) return -1;
    if (hipMemcpyAsync(out, e->c->in.lv.record(e->c->S), 32 * (size_t)e->c->S, hipMemcpyDeviceToHost, e->c->stream) != hipSuccess) return -1;
    return hipStreamSynchronize(e->c->stream) == hipSuccess ? 0 : -1;
}
// The scene-cut detector (DESIGN.md §5.14; scenecut.hip; the checks: picture_host.h): n frames, one launch
int h264mi_scenecut_ok(const h264mi_scenecut *p) { return scenecut_ok(p) ? 0 : -1; }
int h264mi_thumb_size(int w, int h, int *tw, int *th) {
    if (!tw || !th || !canvas_ok(w, h)) return -1;
    *tw = thumb_side(w); *th = thumb_side(h);
    return 0;
}
int h264mi_scenecut_is_cut(const h264mi_scenecut *p, const uint32_t stats[8]) {
    if (!stats || !scenecut_ok(p)) return -1;
    return scenecut_is_cut(p->share, stats[0], stats[1]) ? 1 : 0;
}
int h264mi_i420_scenecut_dev(void *d_stats, void *d_thumb_out, const void *d_cur, const void *d_thumb_prev, int w, int h, int n,
                             const h264mi_scenecut *p, void *hip_stream) {
    if (!scenecut_args_ok(d_stats, d_thumb_out, d_cur, d_thumb_prev, w, h, n, p)) return -1;
    return launch_scenecut_i420((uint32_t *)d_stats, (uint8_t *)d_thumb_out, (const uint8_t *)d_cur, (const uint8_t *)d_thumb_prev, w, h, n, *p,
                                (hipStream_t)hip_stream);
}
int h264mi_enc_set_scenecut(h264mi_encoder *e, const h264mi_scenecut *p) { return e ? enc_set_scenecut(e->c, p) : -1; }
int h264mi_enc_scenecut(h264mi_encoder *e, h264mi_scenecut *out) { return e ? stage_get(e->c->in.sc, out) : -1; }
int h264mi_enc_scenecut_state(h264mi_encoder *e, int stream, uint32_t *out16) {
    if (!e || !out16 || !e->c->in.sc.on || stream < 0 || stream >= e->c->S) return -1;
    if (hipMemcpyAsync(out16, e->c->in.sc.d_words + 16 * (size_t)stream, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, e->c->stream) != hipSuccess) return -1;
    return hipStreamSynchronize(e->c->stream) == hipSuccess ? 0 : -1;
}
// Sprites from RGBA and the standalone blend (DESIGN.md §5.6; overlay.hip)
int h264mi_rgba_to_i420a_dev(void *d_dst, const void *d_rgba, int w, int h, int n, void *hip_stream) {
    if (!d_dst || !d_rgba || ((uintptr_t)d_rgba & 3) || !rgba_to_i420a_args_ok(w, h, n)) return -1;
    return launch_rgba_to_i420a((const uint8_t *)d_rgba, w, h, n, (uint8_t *)d_dst, (hipStream_t)hip_stream);
}
int h264mi_i420_overlay_dev(void *d_canvas, int cw, int ch, int ncanvas, const void *d_sprites, int ow, int oh, int nsprites,
                            const h264mi_overlay *ov, int nov, void *hip_stream) {
    if (!d_canvas || !d_sprites || !overlay_args_ok(cw, ch, ncanvas, ow, oh, nsprites, ov, nov) ||
        byte_ranges_overlap(d_canvas, ncanvas * i420_bytes(cw, ch), d_sprites, nsprites * i420a_bytes(ow, oh)))
        return -1;
    return launch_overlay_i420((uint8_t *)d_canvas, cw, ch, (const uint8_t *)d_sprites, ow, oh, ov, nov, (hipStream_t)hip_stream);
}
// nstreams tight RGBA8 frames back to back: one batched conversion into the encoder's own input area on its
// stream, then the frame step as h264mi_enc_encode runs it
int h264mi_enc_encode_rgba(h264mi_encoder *e, const void *d_rgba_frames) {
    if (!e || !d_rgba_frames || ((uintptr_t)d_rgba_frames & 3)) return -1;
    EncCtx *c = e->c;
    if (colorspec_default(c->cs)) {
        if (launch_rgba_to_i420((const uint8_t *)d_rgba_frames, c->w, c->h, c->S, c->d_src, c->stream) != 0) return -1;
    } else if (!canvas_ok(c->w, c->h) ||
               launch_rgba_to_i420_cs(c->d_src, (const uint8_t *)d_rgba_frames, c->w, c->h, c->S, c->cs, false, c->stream) != 0)
        return -1;
    return enc_code_input(c);
}
// Colour specifications (DESIGN.md §5.11; colorspace.hip; the table and the checks: picture_host.h): n frames, one launch
int h264mi_colorspec_ok(const h264mi_colorspec *spec) { return colorspec_ok(spec) ? 0 : -1; }
static bool cs_rgba_call_ok(const void *d_yuv, size_t yuv_bytes, const void *d_rgba, int w, int h, int n, const h264mi_colorspec *spec) {
    return d_yuv && d_rgba && cs_args_ok(w, h, n, spec) && !((uintptr_t)d_rgba & 3) &&
           !byte_ranges_overlap(d_yuv, (size_t)n * yuv_bytes, d_rgba, (size_t)n * w * h * 4);
}
int h264mi_rgba_to_i420_cs_dev(void *d_i420, const void *d_rgba, int w, int h, int n, const h264mi_colorspec *spec, void *hip_stream) {
    if (!cs_rgba_call_ok(d_i420, i420_bytes(w, h), d_rgba, w, h, n, spec)) return -1;
    return launch_rgba_to_i420_cs((uint8_t *)d_i420, (const uint8_t *)d_rgba, w, h, n, *spec, false, (hipStream_t)hip_stream);
}
int h264mi_i420_to_rgba_cs_dev(void *d_rgba, const void *d_i420, int w, int h, int n, const h264mi_colorspec *spec, void *hip_stream) {
    if (!cs_rgba_call_ok(d_i420, i420_bytes(w, h), d_rgba, w, h, n, spec)) return -1;
    return launch_i420_to_rgba_cs((uint8_t *)d_rgba, (const uint8_t *)d_i420, w, h, n, *spec, (hipStream_t)hip_stream);
}
int h264mi_rgba_to_i420a_cs_dev(void *d_dst, const void *d_rgba, int w, int h, int n, const h264mi_colorspec *spec, void *hip_stream) {
    if (!cs_rgba_call_ok(d_dst, i420a_bytes(w, h), d_rgba, w, h, n, spec)) return -1;
    return launch_rgba_to_i420_cs((uint8_t *)d_dst, (const uint8_t *)d_rgba, w, h, n, *spec, true, (hipStream_t)hip_stream);
}
// what the next h264mi_enc_encode_rgba converts under; a refused one leaves the previous in force
int h264mi_enc_set_colorspec(h264mi_encoder *e, const h264mi_colorspec *spec) {
    if (!e || (spec && !colorspec_ok(spec))) return -1;
    e->c->cs = spec ? *spec : h264mi_colorspec{};
    return 0;
}
int h264mi_enc_colorspec(h264mi_encoder *e, h264mi_colorspec *out) {
    if (!e || !out) return -1;
    *out = e->c->cs;
    return 0;
}
// Area-average downscaling (DESIGN.md §5.3; scale.hip): n tight I420 frames of one geometry pair, one launch
int h264mi_i420_scale_dev(void *d_dst, int dw, int dh, const void *d_src, int sw, int sh, int n, void *hip_stream) {
    if (!d_dst || !d_src || !scale_args_ok(dw, dh, sw, sh, n) || i420_ranges_overlap(d_dst, dw, dh, n, d_src, sw, sh, n)) return -1;
    return launch_scale_i420((uint8_t *)d_dst, dw, dh, (const uint8_t *)d_src, sw, sh, n, (hipStream_t)hip_stream);
}
// nstreams tight src_w x src_h I420 frames back to back: one batched downscale into the encoder's own input area on
// its stream, then the frame step as h264mi_enc_encode runs it (the quality records then see the scaled source).
// Every refusal comes before the first launch
int h264mi_enc_encode_scaled(h264mi_encoder *e, const void *d_frames, int src_w, int src_h) {
    if (!e || !d_frames || enc_resampling_refused(e->c)) return -1;
    EncCtx *c = e->c;
    if (!scale_args_ok(c->w, c->h, src_w, src_h, c->S) || i420_ranges_overlap(c->d_src, c->w, c->h, c->S, d_frames, src_w, src_h, c->S))
        return -1;
    if (launch_scale_i420(c->d_src, c->w, c->h, (const uint8_t *)d_frames, src_w, src_h, c->S, c->stream) != 0) return -1;
    return enc_code_input(c);
}
// Rotating and mirroring (DESIGN.md §5.9; orient.hip): n tight I420 frames of one geometry, one launch
int h264mi_orient_size(int orient, int sw, int sh, int *dw, int *dh) { return orient_size(orient, sw, sh, dw, dh); }
int h264mi_orient_compose(int first, int then) { return orient_compose(first, then); }
int h264mi_orient_inverse(int orient) { return orient_inverse(orient); }
int h264mi_i420_orient_dev(void *d_dst, const void *d_src, int sw, int sh, int n, int orient, void *hip_stream) {
    int dw, dh;
    if (!d_dst || !d_src || !orient_args_ok(orient, sw, sh, n) || orient_size(orient, sw, sh, &dw, &dh) != 0 ||
        i420_ranges_overlap(d_dst, dw, dh, n, d_src, sw, sh, n))
        return -1;
    return launch_orient_i420((uint8_t *)d_dst, (const uint8_t *)d_src, sw, sh, n, orient, (hipStream_t)hip_stream);
}
// nstreams tight I420 frames back to back that orient turns into the encoder's pictures (h x w ones for a transposing
// orientation): one batched launch into the encoder's own input area on its stream, then the frame step as
// h264mi_enc_encode runs it. Every refusal comes before the first launch
int h264mi_enc_encode_oriented(h264mi_encoder *e, const void *d_frames, int orient) {
    if (!e || !d_frames || enc_resampling_refused(e->c)) return -1;
    EncCtx *c = e->c;
    int sw, sh;  // the inverse turns a w x h picture back into the source's size
    if (orient_size(orient_inverse(orient), c->w, c->h, &sw, &sh) != 0 || !orient_args_ok(orient, sw, sh, c->S) ||
        i420_ranges_overlap(c->d_src, c->w, c->h, c->S, d_frames, sw, sh, c->S))
        return -1;
    if (launch_orient_i420(c->d_src, (const uint8_t *)d_frames, sw, sh, c->S, orient, c->stream) != 0) return -1;
    return enc_code_input(c);
}
// The mesh warp (DESIGN.md §5.20; warp.hip; the checks: picture_host.h): n frames, one launch up to 2^30 tiles
int h264mi_warp_ok(const h264mi_warp *p) { return warp_ok(p) ? 0 : -1; }
int h264mi_warp_mesh_size(int dw, int dh, int grid_log2, int *mw, int *mh) {
    if (!mw || !mh || !canvas_ok(dw, dh) || !warp_grid_ok(grid_log2)) return -1;
    *mw = warp_mesh_side(dw, grid_log2); *mh = warp_mesh_side(dh, grid_log2);
    return 0;
}
int h264mi_warp_mesh_affine(int32_t *mesh, int dw, int dh, int grid_log2, const int32_t m[6]) { return warp_mesh_affine(mesh, dw, dh, grid_log2, m); }
int h264mi_warp_mesh_homography(int32_t *mesh, int dw, int dh, int grid_log2, const int32_t h[9]) {
    return warp_mesh_homography(mesh, dw, dh, grid_log2, h);
}
int h264mi_warp_mesh_radial(int32_t *mesh, int dw, int dh, int grid_log2, int cx, int cy, int64_t r2, int k1, int k2) {
    return warp_mesh_radial(mesh, dw, dh, grid_log2, cx, cy, r2, k1, k2);
}
int h264mi_warp_tile_class(const int32_t *mesh, int dw, int dh, int sw, int sh, int grid_log2, int plane, int tx, int ty) {
    return warp_tile_class(mesh, dw, dh, sw, sh, grid_log2, plane, tx, ty);
}
int h264mi_i420_warp_dev(void *d_dst, int dw, int dh, const void *d_src, int sw, int sh, int n, const void *d_mesh, int mesh_per_frame,
                         const h264mi_warp *p, void *hip_stream) {
    if (!warp_args_ok(d_dst, dw, dh, d_src, sw, sh, n, d_mesh, mesh_per_frame, p)) return -1;
    return launch_warp_i420((uint8_t *)d_dst, dw, dh, (const uint8_t *)d_src, sw, sh, n, (const int32_t *)d_mesh, mesh_per_frame, *p, 0,
                            (hipStream_t)hip_stream);
}
int h264mi_i420_warp_host(void *dst, int dw, int dh, const void *src, int sw, int sh, const int32_t *mesh, const h264mi_warp *p) {
    if (!warp_args_ok(dst, dw, dh, src, sw, sh, 1, mesh, 0, p)) return -1;
    warp_frame_host((uint8_t *)dst, dw, dh, (const uint8_t *)src, sw, sh, mesh, *p);
    return 0;
}
// nstreams tight src_w x src_h I420 frames back to back: one batched warp into the encoder's own input area on its
// stream, then the frame step as h264mi_enc_encode runs it. Every refusal comes before the first launch
int h264mi_enc_encode_warped(h264mi_encoder *e, const void *d_frames, int src_w, int src_h, const void *d_mesh, int mesh_per_stream,
                             const h264mi_warp *p) {
    if (!e || enc_resampling_refused(e->c)) return -1;
    EncCtx *c = e->c;
    if (!warp_args_ok(c->d_src, c->w, c->h, d_frames, src_w, src_h, c->S, d_mesh, mesh_per_stream, p)) return -1;
    if (launch_warp_i420(c->d_src, c->w, c->h, (const uint8_t *)d_frames, src_w, src_h, c->S, (const int32_t *)d_mesh, mesh_per_stream, *p, 0,
                         c->stream) != 0)
        return -1;
    return enc_code_input(c);
}
// measurement only (tools/warp_ab.py), not declared in the header: h264mi_i420_warp_dev with the path of this one
// call given -- 0 as the call chooses, 1 every tile from global memory. No state is kept
int h264mi_i420_warp_path_dev(void *d_dst, int dw, int dh, const void *d_src, int sw, int sh, int n, const void *d_mesh, int mesh_per_frame,
                              const h264mi_warp *p, int path, void *hip_stream);
int h264mi_i420_warp_path_dev(void *d_dst, int dw, int dh, const void *d_src, int sw, int sh, int n, const void *d_mesh, int mesh_per_frame,
                              const h264mi_warp *p, int path, void *hip_stream) {
    if (!warp_args_ok(d_dst, dw, dh, d_src, sw, sh, n, d_mesh, mesh_per_frame, p) || (path != 0 && path != 1)) return -1;
    return launch_warp_i420((uint8_t *)d_dst, dw, dh, (const uint8_t *)d_src, sw, sh, n, (const int32_t *)d_mesh, mesh_per_frame, *p, path,
                            (hipStream_t)hip_stream);
}
// Pixel formats and pitched layouts (DESIGN.md §5.10; pixfmt.hip; the rules: picture_host.h): n frames, one launch
int h264mi_pix_layout_tight(h264mi_pix_layout *out, int pix, int w, int h) { return pix_layout_tight(out, pix, w, h); }
int64_t h264mi_pix_span(const h264mi_pix_layout *layout, int w, int h) { return pix_span(layout, w, h); }
int h264mi_pix_layout_ok(const h264mi_pix_layout *layout, int w, int h) { return pix_layout_ok(layout, w, h) ? 0 : -1; }
int h264mi_pix_unit(int pix) { return pix_unit(pix); }
int h264mi_pixopt_ok(const h264mi_pixopt *opt) { return pixopt_ok(opt) ? 0 : -1; }
// the formats 16..24 go to pixdeep.hip (DESIGN.md §5.17), under the depth rule of opt; the others never look at it
int h264mi_pix_to_i420_opt_dev(void *d_i420, const void *d_src, const h264mi_pix_layout *src, const h264mi_pixopt *opt, int w, int h, int n,
                               void *hip_stream) {
    if (!d_i420 || !d_src || (opt && !pixopt_ok(opt)) || !pix_args_ok(src, w, h, n) || !pix_base_ok(d_src, *src) ||
        pix_ranges_overlap(d_src, *src, d_i420, w, h, n))
        return -1;
    return launch_layout_to_i420((uint8_t *)d_i420, (const uint8_t *)d_src, *src, opt ? opt->depth : 0, w, h, n, (hipStream_t)hip_stream);
}
int h264mi_pix_to_i420_dev(void *d_i420, const void *d_src, const h264mi_pix_layout *src, int w, int h, int n, void *hip_stream) {
    return h264mi_pix_to_i420_opt_dev(d_i420, d_src, src, nullptr, w, h, n, hip_stream);
}
int h264mi_i420_to_pix_dev(void *d_dst, const h264mi_pix_layout *dst, const void *d_i420, int w, int h, int n, void *hip_stream) {
    if (!d_dst || !d_i420 || !pix_args_ok(dst, w, h, n) || !pix_base_ok(d_dst, *dst) || pix_ranges_overlap(d_dst, *dst, d_i420, w, h, n)) return -1;
    return launch_i420_to_layout((uint8_t *)d_dst, *dst, (const uint8_t *)d_i420, w, h, n, (hipStream_t)hip_stream);
}
// nstreams frames of the encoder's size in *layout: one batched launch into the encoder's own input area on its stream,
// then the frame step as h264mi_enc_encode runs it. Every refusal comes before the first launch
int h264mi_enc_encode_pix(h264mi_encoder *e, const void *d_frames, const h264mi_pix_layout *layout) {
    if (!e || !d_frames) return -1;
    EncCtx *c = e->c;
    if (!pix_args_ok(layout, c->w, c->h, c->S) || !pix_base_ok(d_frames, *layout) ||
        pix_ranges_overlap(d_frames, *layout, c->d_src, c->w, c->h, c->S))
        return -1;
    if (launch_layout_to_i420(c->d_src, (const uint8_t *)d_frames, *layout, c->pixopt.depth, c->w, c->h, c->S, c->stream) != 0) return -1;
    return enc_code_input(c);
}
// the depth rule the next h264mi_enc_encode_pix converts under; a refused one leaves the previous in force
int h264mi_enc_set_pixopt(h264mi_encoder *e, const h264mi_pixopt *opt) {
    if (!e || (opt && !pixopt_ok(opt))) return -1;
    e->c->pixopt = opt ? *opt : h264mi_pixopt{};
    return 0;
}
int h264mi_enc_pixopt(h264mi_encoder *e, h264mi_pixopt *out) {
    if (!e || !out) return -1;
    *out = e->c->pixopt;
    return 0;
}
// Several pictures into one (DESIGN.md §5.4; compose.hip): every cell's crop of a source frame area-averaged into its
// rectangle of a canvas, 64 cells to a launch
int h264mi_i420_compose_dev(void *d_canvas, int cw, int ch, int ncanvas, const void *d_src, int src_w, int src_h, int nsrc,
                            const h264mi_cell *cells, int ncells, void *hip_stream) {
    if (!d_canvas || !d_src || !cells_ok(cw, ch, ncanvas, src_w, src_h, nsrc, cells, ncells, false) ||
        i420_ranges_overlap(d_canvas, cw, ch, ncanvas, d_src, src_w, src_h, nsrc))
        return -1;
    return launch_compose_i420((uint8_t *)d_canvas, cw, ch, (const uint8_t *)d_src, src_w, src_h, cells, ncells, (hipStream_t)hip_stream);
}
int h264mi_i420_fill_dev(void *d_frames, int w, int h, int n, int y, int cb, int cr, void *hip_stream) {
    if (!d_frames || !fill_args_ok(w, h, n, y, cb, cr)) return -1;
    return launch_fill_i420((uint8_t *)d_frames, w, h, n, y, cb, cr, (hipStream_t)hip_stream);
}
int h264mi_mosaic_cells(h264mi_cell *out, int cap, int n, int src_w, int src_h, int cw, int ch) {
    return mosaic_cells(out, cap, n, src_w, src_h, cw, ch);
}
// the encoder's nstreams input frames as the canvases: an optional fill, the compose launch(es), then the frame step
// as h264mi_enc_encode runs it, all on the encoder's stream. With may_enlarge the cells may enlarge, with filter.
// Every refusal comes before the first launch
static int enc_encode_cells(h264mi_encoder *e, const void *d_src, int src_w, int src_h, int nsrc, const h264mi_cell *cells, int ncells,
                            bool may_enlarge, int filter, int bg_y, int bg_cb, int bg_cr) {
    if (!e || !d_src || enc_resampling_refused(e->c)) return -1;
    EncCtx *c = e->c;
    if ((may_enlarge && !filter_ok(filter)) || !cells_ok(c->w, c->h, c->S, src_w, src_h, nsrc, cells, ncells, may_enlarge) ||
        i420_ranges_overlap(c->d_src, c->w, c->h, c->S, d_src, src_w, src_h, nsrc))
        return -1;
    if (bg_y > 255 || bg_cb > 255 || bg_cr > 255 || (bg_y >= 0 && !fill_args_ok(c->w, c->h, c->S, bg_y, bg_cb, bg_cr))) return -1;
    if (bg_y >= 0 && launch_fill_i420(c->d_src, c->w, c->h, c->S, bg_y, bg_cb, bg_cr, c->stream) != 0) return -1;
    const uint8_t *src = (const uint8_t *)d_src;
    const int rc = may_enlarge ? launch_compose_any_i420(c->d_src, c->w, c->h, src, src_w, src_h, cells, ncells, filter, c->stream)
                               : launch_compose_i420(c->d_src, c->w, c->h, src, src_w, src_h, cells, ncells, c->stream);
    return rc != 0 ? -1 : enc_code_input(c);
}
int h264mi_enc_encode_composed(h264mi_encoder *e, const void *d_src, int src_w, int src_h, int nsrc, const h264mi_cell *cells, int ncells,
                               int bg_y, int bg_cb, int bg_cr) {
    return enc_encode_cells(e, d_src, src_w, src_h, nsrc, cells, ncells, false, 0, bg_y, bg_cb, bg_cr);
}
// Enlarging (DESIGN.md §5.7; upscale.hip): whole frames, cells of both kinds, the active-speaker layout
int h264mi_i420_upscale_dev(void *d_dst, int dw, int dh, const void *d_src, int sw, int sh, int n, int filter, void *hip_stream) {
    if (!d_dst || !d_src || !upscale_args_ok(dw, dh, sw, sh, n, filter) || i420_ranges_overlap(d_dst, dw, dh, n, d_src, sw, sh, n))
        return -1;
    return launch_upscale_i420((uint8_t *)d_dst, dw, dh, (const uint8_t *)d_src, sw, sh, n, filter, (hipStream_t)hip_stream);
}
int h264mi_i420_compose_any_dev(void *d_canvas, int cw, int ch, int ncanvas, const void *d_src, int src_w, int src_h, int nsrc,
                                const h264mi_cell *cells, int ncells, int filter, void *hip_stream) {
    if (!d_canvas || !d_src || !filter_ok(filter) || !cells_ok(cw, ch, ncanvas, src_w, src_h, nsrc, cells, ncells, true) ||
        i420_ranges_overlap(d_canvas, cw, ch, ncanvas, d_src, src_w, src_h, nsrc))
        return -1;
    return launch_compose_any_i420((uint8_t *)d_canvas, cw, ch, (const uint8_t *)d_src, src_w, src_h, cells, ncells, filter,
                                   (hipStream_t)hip_stream);
}
int h264mi_speaker_cells(h264mi_cell *out, int cap, int n, int speaker, int src_w, int src_h, int cw, int ch) {
    return speaker_cells(out, cap, n, speaker, src_w, src_h, cw, ch);
}
// h264mi_enc_encode_composed with cells that may enlarge
int h264mi_enc_encode_composed_any(h264mi_encoder *e, const void *d_src, int src_w, int src_h, int nsrc, const h264mi_cell *cells, int ncells,
                                   int filter, int bg_y, int bg_cb, int bg_cr) {
    return enc_encode_cells(e, d_src, src_w, src_h, nsrc, cells, ncells, true, filter, bg_y, bg_cb, bg_cr);
}
const void *h264mi_enc_input_buffer(h264mi_encoder *e) { return e ? e->c->d_src : nullptr; }
size_t h264mi_enc_frame_bytes(h264mi_encoder *e) { return e ? e->c->fbytes : 0; }
size_t h264mi_enc_rgba_frame_bytes(h264mi_encoder *e) { return e ? (size_t)e->c->w * e->c->h * 4 : 0; }
int h264mi_enc_sync(h264mi_encoder *e) { return e && hipStreamSynchronize(e->c->stream) == hipSuccess ? 0 : -1; }
int h264mi_enc_nal_bytes(h264mi_encoder *e, int *out) {
    if (!e) return -1;
    std::vector<EncState> st(e->c->S);
    if (hipMemcpyAsync(st.data(), e->c->d_st, sizeof(EncState) * e->c->S, hipMemcpyDeviceToHost, e->c->stream) != hipSuccess) return -1;
    if (hipStreamSynchronize(e->c->stream) != hipSuccess) return -1;
    int err = 0;
    for (int s = 0; s < e->c->S; s++) { out[s] = st[s].nal_bytes; err |= st[s].err; }
    return err ? -2 : 0;
}
const void *h264mi_enc_nal_ptr(h264mi_encoder *e, int stream) {
    if (!e || stream < 0 || stream >= e->c->S) return nullptr;
    return e->c->h_desc[e->c->parity ^ 1][stream].nal;
}
const void *h264mi_enc_recon_ptr(h264mi_encoder *e, int stream) {
    if (!e || stream < 0 || stream >= e->c->S) return nullptr;
    return e->c->h_desc[e->c->parity ^ 1][stream].dbk[0];
}
int h264mi_enc_ref_planes(h264mi_encoder *e, int stream, void *host_out) {
    if (!e || stream < 0 || stream >= e->c->S) return -1;
    const EncDesc &d = e->c->h_desc[0][stream];
    const size_t lsz = (size_t)d.ps * (e->c->ch + 2 * H264MI_LPADY), csz = (size_t)d.psc * (e->c->ch / 2 + 2 * H264MI_CPADY);
    uint8_t *o = (uint8_t *)host_out;
    if (hipStreamSynchronize(e->c->stream) != hipSuccess) return -1;
    for (int k = 0; k < 4; k++)
        if (hipMemcpy(o + k * lsz, d.pl[k] - (size_t)H264MI_LPADY * d.ps - H264MI_LPADX, lsz, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    for (int k = 0; k < 2; k++)
        if (hipMemcpy(o + 4 * lsz + k * csz, d.plc[k] - (size_t)H264MI_CPADY * d.psc - H264MI_CPADX, csz, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return 0;
}
int h264mi_enc_last_qp(h264mi_encoder *e, int stream) {
    if (!e || stream < 0 || stream >= e->c->S) return -1;
    EncState st;
    if (hipMemcpy(&st, e->c->d_st + stream, sizeof(EncState), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return st.cur_qp;
}
int h264mi_enc_rc_state(h264mi_encoder *e, int stream, int *out) {
    if (!e || !out || stream < 0 || stream >= e->c->S) return -1;
    EncState st;
    if (hipStreamSynchronize(e->c->stream) != hipSuccess) return -1;
    if (hipMemcpy(&st, e->c->d_st + stream, sizeof(EncState), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    const RcState &r = st.rc;
    const int v[16] = {st.cur_skip, st.cur_qp, r.avg_qp, r.target, r.remaining, (int)r.fullness, r.continual_skip,
                       (int)r.frame_cmplx, r.min_frame_qp, r.max_frame_qp, r.bpf, r.pframe_num, r.idr_num, r.skip_flag,
                       r.remaining_weights, r.frame_coded_in_vgop};
    memcpy(out, v, sizeof(v));
    return 0;
}
int h264mi_enc_gom_state(h264mi_encoder *e, int stream, int *out, int cap) {
    if (!e || stream < 0 || stream >= e->c->S) return -1;
    const int G = e->c->gom_count;
    if (!out || !e->c->gom_exact) return G;
    if (hipStreamSynchronize(e->c->stream) != hipSuccess) return -1;
    std::vector<uint64_t> g(4 * (size_t)G);
    if (hipMemcpy(g.data(), e->c->h_desc[0][stream].gomst, 8 * g.size(), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    for (int i = 0; i < 4 * G && i < cap; i++) out[i] = (int)(uint32_t)g[i];
    return G;
}
int h264mi_rc_qstep_to_qp(int qstep) {
    static const int32_t thr[52] = {H264MI_RC_QP_THR_LIST};
    if (qstep < 64) return 0;
    int q = 0;
    while (q < 52 && qstep >= thr[q]) q++;
    return q;
}
int h264mi_enc_mbinfo(h264mi_encoder *e, int stream, void *host_out) {
    if (!e || stream < 0 || stream >= e->c->S) return -1;
    return hipMemcpy(host_out, e->c->h_desc[0][stream].info, sizeof(MbInfo) * e->c->nmb, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
void *h264mi_enc_stream(h264mi_encoder *e) { return e ? (void *)e->c->stream : nullptr; }
const int *h264mi_enc_nal_size_dev(h264mi_encoder *e, int stream) {
    if (!e || stream < 0 || stream >= e->c->S) return nullptr;
    return &e->c->d_st[stream].nal_bytes;
}
int h264mi_enc_copy_nals(h264mi_encoder *e, void *d_dst, int slot_bytes, int *d_sizes) {
    if (!e || !d_dst || slot_bytes <= 0 || (slot_bytes & 3)) return -1;
    EncCtx *c = e->c;
    hipLaunchKernelGGL(enc_copy_nals_kernel, dim3(64, c->S), dim3(256), 0, c->stream,
                       PackNalLaunch{c->S, c->d_desc[c->parity ^ 1], (uint8_t *)d_dst, slot_bytes, (int32_t *)d_sizes});
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int h264mi_enc_profile(h264mi_encoder *e, uint64_t *out) {
    if (!e || !e->c->d_prof) return -1;
    return hipMemcpy(out, e->c->d_prof, 64 * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
const uint32_t *h264mi_enc_rows_counter(h264mi_encoder *e) { return e ? e->c->d_ticket + 32 : nullptr; }
int h264mi_enc_timeline(h264mi_encoder *e, uint64_t *out, int n) {
    if (!e || !e->c->d_tl || n < 4 * e->c->S * e->c->mbh) return -1;
    return hipMemcpy(out, e->c->d_tl, 4 * (size_t)e->c->S * e->c->mbh * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
int h264mi_enc_set_timing(h264mi_encoder *e, int enable) {
    if (!e) return -1;
    if (hipStreamSynchronize(e->c->stream) != hipSuccess) return -1;
    e->c->timing = enable != 0;
    e->c->ev_used = 0;
    return 0;
}
// total ms and launch count of enc_mb_kernel since set_timing (synchronises)
int h264mi_enc_kernel_time(h264mi_encoder *e, double *ms_total, int *launches) {
    if (!e) return -1;
    EncCtx *c = e->c;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    double t = 0;
    for (int i = 0; i + 1 < c->ev_used; i += 2) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]) != hipSuccess) return -1;
        t += ms;
    }
    *ms_total = t;
    *launches = c->ev_used / 2;
    return 0;
}

}  // extern "C"
