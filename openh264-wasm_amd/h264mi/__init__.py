"""h264mi -- Python host bindings of libh264mi (MI355X-native H.264 encode/decode core).

Layering:
  * ``lib/libh264mi.so`` -- HIP kernels for gfx950 + runtime + the C-ABI declared in
    ``include/h264mi.h``.
  * ``Module`` (this file) -- mirrors the Emscripten ``Module`` object the reference's workers use
    (``cwrap``/``_malloc``/``_free``/``getValue``/``HEAPU8``; scripts/encoder_worker.js:27-29,
    decoder_worker.js:346-349) so call sequences read exactly like the reference's glue.
  * ``BatchEncoder`` / ``BatchDecoder`` -- the device-resident multi-stream API (frames and NAL
    units already in HBM) used by bench.py and the multi-GPU path.

There is no CPU fallback: importing this module on a machine without the built library raises.
"""
import atexit
import ctypes
import os
import sys
import weakref

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('H264MI_LIB') or os.path.join(os.path.dirname(_HERE), 'lib', 'libh264mi.so')  # env: diagnostics

_lib = None


def lib():
    """Load libh264mi.so (fails loudly when it is missing -- there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f'libh264mi.so not built ({LIB_PATH}); run openh264-wasm_amd/build.py')
        L = ctypes.CDLL(LIB_PATH)
        vp, i, cp = ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p
        sig = {
            'init_encoder': (i, [i, i, i]),
            'force_key_frame': (None, []),
            'init_decoder': (i, [i]),
            'deinit_decoder': (None, [i]),
            'encode_frame': (None, [vp, i, i, vp, vp]),
            'encode_frame_yuv_i420': (None, [vp, i, i, vp, vp]),
            'decode_frame_optimized': (None, [i, vp, i, vp, vp, vp]),
            'decode_frame_yuv_i420': (None, [i, vp, i, vp, vp, vp]),
            'free_buffer': (None, [vp]),
            'h264mi_enc_create': (vp, [i, i, i, i, vp]),
            'h264mi_enc_destroy': (None, [vp]),
            'h264mi_enc_force_idr': (i, [vp, i]),
            'h264mi_enc_encode': (i, [vp, vp]),
            'h264mi_enc_set_frame_skip': (i, [vp, i]),
            'h264mi_enc_frames_skipped': (i, [vp, i]),
            'h264mi_enc_set_gom_exact': (i, [vp, i]),
            'h264mi_enc_set_slices': (i, [vp, i]),
            'h264mi_enc_slices': (i, [vp]),
            'h264mi_slice_first_row': (i, [i, i, i]),
            'h264mi_enc_inject_error': (i, [vp, i, i]),
            'h264mi_enc_sync': (i, [vp]),
            'h264mi_enc_nal_bytes': (i, [vp, vp]),
            'h264mi_enc_nal_ptr': (vp, [vp, i]),
            'h264mi_enc_recon_ptr': (vp, [vp, i]),
            'h264mi_enc_input_buffer': (vp, [vp]),
            'h264mi_enc_frame_bytes': (ctypes.c_size_t, [vp]),
            'h264mi_enc_last_qp': (i, [vp, i]),
            'h264mi_enc_rc_state': (i, [vp, i, vp]),
            'h264mi_enc_gom_state': (i, [vp, i, vp, i]),
            'h264mi_rc_qstep_to_qp': (i, [i]),
            'h264mi_enc_mbinfo': (i, [vp, i, vp]),
            'h264mi_enc_ref_planes': (i, [vp, i, vp]),
            'h264mi_enc_stream': (vp, [vp]),
            'h264mi_enc_nal_size_dev': (vp, [vp, i]),
            'h264mi_enc_copy_nals': (i, [vp, vp, i, vp]),
            'h264mi_enc_set_timing': (i, [vp, i]),
            'h264mi_enc_kernel_time': (i, [vp, vp, vp]),
            'h264mi_dec_decode_dev': (i, [vp, vp, vp]),
            'h264mi_dec_create': (vp, [i, i, i, vp]),
            'h264mi_dec_destroy': (None, [vp]),
            'h264mi_dec_create_batch': (vp, [i, i, i, i, vp]),
            'h264mi_dec_create_ring': (vp, [i, i, i, i, i, i, vp]),
            'h264mi_dec_device_bytes': (ctypes.c_size_t, [vp]),
            'h264mi_dec_ring_groups': (i, [vp]),
            'h264mi_i_decoder_device_bytes': (ctypes.c_size_t, [vp, i]),
            'h264mi_instance_create': (vp, []),
            'h264mi_instance_destroy': (None, [vp]),
            'h264mi_dec_decode_frames': (i, [vp, i, vp, vp, vp]),
            'h264mi_dec_decode_frames_after': (i, [vp, i, vp, vp, vp, vp]),
            'h264mi_dec_decode_frames_after_n': (i, [vp, i, vp, vp, vp, vp, i]),
            'h264mi_dec_decode_frames_out': (i, [vp, i, vp, vp, vp, vp, i, vp, vp]),
            'h264mi_dec_recon_profile': (i, [vp, vp]),
            'h264mi_dec_max_frames': (i, [vp]),
            'h264mi_dec_set_parse_streams': (i, [vp, i]),
            'h264mi_dec_set_slice_waves': (i, [vp, i]),
            'h264mi_dec_set_streamed': (i, [vp, i]),
            'h264mi_dec_streamed': (i, [vp]),
            'h264mi_dec_set_resolve': (i, [vp, i]),
            'h264mi_dec_resolve_launches': (ctypes.c_longlong, [vp]),
            'h264mi_dec_set_conceal': (i, [vp, i]),
            'h264mi_dec_conceal': (i, [vp]),
            'h264mi_dec_concealed': (i, [vp, vp]),
            'h264mi_dec_concealed_ptr': (vp, [vp]),
            'h264mi_conceal_gaps': (i, [i, i, vp, vp, vp, vp, i]),
            'h264mi_dec_set_streamed_budget': (i, [i]),
            'h264mi_nal_pack': (i, [vp, vp, ctypes.c_size_t, vp, i, vp]),
            'h264mi_nal_unpack': (i, [vp, vp, ctypes.c_size_t, vp, i, vp]),
            'h264mi_dec_set_parse_cus': (i, [vp, i, i]),
            'h264mi_stream_create_cus': (vp, [i, i, i]),
            'h264mi_stream_destroy': (None, [vp]),
            'h264mi_dec_decode': (i, [vp, vp, vp]),
            'h264mi_dec_sync': (i, [vp]),
            'h264mi_dec_set_timing': (i, [vp, i]),
            'h264mi_dec_kernel_time': (i, [vp, i, vp, vp]),
            'h264mi_dec_status': (i, [vp, vp]),
            'h264mi_dec_parse_profile': (i, [vp, vp]),
            'h264mi_enc_profile': (i, [vp, vp]),
            'h264mi_enc_timeline': (i, [vp, vp, i]),
            'h264mi_dec_picture_ptr': (vp, [vp, i]),
            'h264mi_dec_coded_size': (i, [vp, vp, vp]),
            'h264mi_dec_stream': (vp, [vp]),
            'h264mi_rgba_to_i420_host': (i, [vp, i, i, vp]),
            'h264mi_i420_to_rgba_host': (i, [vp, i, i, vp]),
            'h264mi_rgba_to_i420_dev': (i, [vp, vp, i, i, i, vp]),
            'h264mi_i420_to_rgba_dev': (i, [vp, vp, i, i, i, vp]),
            'h264mi_enc_encode_rgba': (i, [vp, vp]),
            'h264mi_enc_rgba_frame_bytes': (ctypes.c_size_t, [vp]),
            'h264mi_dec_set_output_format': (i, [vp, i]),
            'h264mi_dec_output_format': (i, [vp]),
            'h264mi_ring_create': (vp, [i, i]),
            'h264mi_ring_destroy': (None, [vp]),
            'h264mi_ring_publish': (ctypes.c_longlong, [vp, vp, i, i]),
            'h264mi_ring_nal_ptr': (vp, [vp, ctypes.c_longlong]),
            'h264mi_ring_size_dev': (vp, [vp, ctypes.c_longlong]),
            'h264mi_ring_release': (i, [vp, ctypes.c_longlong, vp]),
            'h264mi_ring_stats': (i, [vp, vp, vp, vp, vp]),
            'h264mi_version': (cp, []),
            'h264mi_enc_rows_counter': (vp, [vp]),
            'h264mi_dec_set_recon_gate': (i, [vp, vp, ctypes.c_uint32, ctypes.c_uint32, i, i]),
            'h264mi_i420_quality_dev': (i, [vp, vp, vp, i, i, i, vp]),
            'h264mi_psnr': (ctypes.c_double, [ctypes.c_uint64, ctypes.c_uint64]),
            'h264mi_enc_set_quality': (i, [vp, i]),
            'h264mi_enc_quality_enabled': (i, [vp]),
            'h264mi_enc_quality': (i, [vp, i, vp]),
            'h264mi_enc_quality_dev': (vp, [vp]),
            'h264mi_i420_scale_dev': (i, [vp, i, i, vp, i, i, i, vp]),
            'h264mi_enc_encode_scaled': (i, [vp, vp, i, i]),
            'h264mi_i420_compose_dev': (i, [vp, i, i, i, vp, i, i, i, vp, i, vp]),
            'h264mi_i420_fill_dev': (i, [vp, i, i, i, i, i, i, vp]),
            'h264mi_mosaic_cells': (i, [vp, i, i, i, i, i, i]),
            'h264mi_enc_encode_composed': (i, [vp, vp, i, i, i, vp, i, i, i, i]),
            'h264mi_rgba_to_i420a_dev': (i, [vp, vp, i, i, i, vp]),
            'h264mi_i420_overlay_dev': (i, [vp, i, i, i, vp, i, i, i, vp, i, vp]),
            'h264mi_enc_set_overlays': (i, [vp, vp, i, i, i, vp, i]),
            'h264mi_enc_overlays': (i, [vp]),
            'h264mi_i420_upscale_dev': (i, [vp, i, i, vp, i, i, i, i, vp]),
            'h264mi_i420_compose_any_dev': (i, [vp, i, i, i, vp, i, i, i, vp, i, i, vp]),
            'h264mi_speaker_cells': (i, [vp, i, i, i, i, i, i, i]),
            'h264mi_enc_encode_composed_any': (i, [vp, vp, i, i, i, vp, i, i, i, i, i]),
            'h264mi_orient_size': (i, [i, i, i, vp, vp]),
            'h264mi_orient_compose': (i, [i, i]),
            'h264mi_orient_inverse': (i, [i]),
            'h264mi_i420_orient_dev': (i, [vp, vp, i, i, i, i, vp]),
            'h264mi_enc_encode_oriented': (i, [vp, vp, i]),
            'h264mi_pix_layout_tight': (i, [vp, i, i, i]),
            'h264mi_pix_span': (ctypes.c_int64, [vp, i, i]),
            'h264mi_pix_layout_ok': (i, [vp, i, i]),
            'h264mi_pix_to_i420_dev': (i, [vp, vp, vp, i, i, i, vp]),
            'h264mi_i420_to_pix_dev': (i, [vp, vp, vp, i, i, i, vp]),
            'h264mi_enc_encode_pix': (i, [vp, vp, vp]),
            'h264mi_pix_unit': (i, [i]),
            'h264mi_pixopt_ok': (i, [vp]),
            'h264mi_pix_to_i420_opt_dev': (i, [vp, vp, vp, vp, i, i, i, vp]),
            'h264mi_enc_set_pixopt': (i, [vp, vp]),
            'h264mi_enc_pixopt': (i, [vp, vp]),
            'h264mi_dec_set_output_layout': (i, [vp, vp]),
            'h264mi_dec_output_layout': (i, [vp, vp]),
            'h264mi_colorspec_ok': (i, [vp]),
            'h264mi_rgba_to_i420_cs_dev': (i, [vp, vp, i, i, i, vp, vp]),
            'h264mi_i420_to_rgba_cs_dev': (i, [vp, vp, i, i, i, vp, vp]),
            'h264mi_rgba_to_i420a_cs_dev': (i, [vp, vp, i, i, i, vp, vp]),
            'h264mi_enc_set_colorspec': (i, [vp, vp]),
            'h264mi_enc_colorspec': (i, [vp, vp]),
            'h264mi_dec_set_output_colorspec': (i, [vp, vp]),
            'h264mi_dec_output_colorspec': (i, [vp, vp]),
            'h264mi_denoise_ok': (i, [vp]),
            'h264mi_i420_denoise_dev': (i, [vp, vp, vp, vp, i, i, i, vp, vp, vp]),
            'h264mi_enc_set_denoise': (i, [vp, vp]),
            'h264mi_enc_denoise': (i, [vp, vp]),
            'h264mi_deinterlace_ok': (i, [vp]),
            'h264mi_i420_deinterlace_dev': (i, [vp, vp, vp, vp, i, i, i, vp, vp, vp]),
            'h264mi_i420_deinterlace_host': (i, [vp, vp, vp, i, i, vp, vp]),
            'h264mi_enc_set_deinterlace': (i, [vp, vp]),
            'h264mi_enc_deinterlace': (i, [vp, vp]),
            'h264mi_scenecut_ok': (i, [vp]),
            'h264mi_thumb_size': (i, [i, i, vp, vp]),
            'h264mi_scenecut_is_cut': (i, [vp, vp]),
            'h264mi_i420_scenecut_dev': (i, [vp, vp, vp, vp, i, i, i, vp, vp]),
            'h264mi_enc_set_scenecut': (i, [vp, vp]),
            'h264mi_enc_scenecut': (i, [vp, vp]),
            'h264mi_enc_scenecut_state': (i, [vp, i, vp]),
            'h264mi_spatial_ok': (i, [vp]),
            'h264mi_i420_spatial_dev': (i, [vp, vp, i, i, i, vp, vp]),
            'h264mi_i420_spatial_host': (i, [vp, vp, i, i, vp]),
            'h264mi_privacy_ok': (i, [vp, i, i, i, i]),
            'h264mi_i420_privacy_dev': (i, [vp, i, i, i, vp, i, vp]),
            'h264mi_i420_privacy_host': (i, [vp, i, i, i, vp, i]),
            'h264mi_enc_set_spatial': (i, [vp, vp]),
            'h264mi_enc_spatial': (i, [vp, vp]),
            'h264mi_enc_set_privacy': (i, [vp, vp, i]),
            'h264mi_enc_privacy': (i, [vp]),
            'h264mi_levels_ok': (i, [vp]),
            'h264mi_i420_hist_dev': (i, [vp, vp, i, i, i, vp]),
            'h264mi_i420_lut_dev': (i, [vp, vp, i, i, i, vp, i, vp]),
            'h264mi_levels_work_bytes': (ctypes.c_size_t, [i]),
            'h264mi_i420_levels_dev': (i, [vp, vp, i, i, i, vp, vp, vp, vp, vp]),
            'h264mi_i420_hist_host': (i, [vp, vp, i, i]),
            'h264mi_i420_lut_host': (i, [vp, vp, i, i, vp]),
            'h264mi_levels_lut_host': (i, [vp, vp, i, i, vp, vp, vp]),
            'h264mi_enc_set_levels': (i, [vp, vp]),
            'h264mi_enc_levels': (i, [vp, vp]),
            'h264mi_enc_levels_record': (i, [vp, vp, i]),
            'h264mi_warp_ok': (i, [vp]),
            'h264mi_warp_mesh_size': (i, [i, i, i, vp, vp]),
            'h264mi_warp_mesh_affine': (i, [vp, i, i, i, vp]),
            'h264mi_warp_mesh_homography': (i, [vp, i, i, i, vp]),
            'h264mi_warp_mesh_radial': (i, [vp, i, i, i, i, i, ctypes.c_int64, i, i]),
            'h264mi_warp_tile_class': (i, [vp, i, i, i, i, i, i, i, i]),
            'h264mi_i420_warp_dev': (i, [vp, i, i, vp, i, i, i, vp, i, vp, vp]),
            'h264mi_i420_warp_host': (i, [vp, i, i, vp, i, i, vp, vp]),
            'h264mi_enc_encode_warped': (i, [vp, vp, i, i, vp, i, vp]),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


# Teardown order. GPU objects (encoders, decoders, rings, CU-masked streams) are released explicitly by
# close(), or at interpreter exit by the atexit hook below -- which runs before the HIP runtime and torch
# unload. __del__ does nothing once the interpreter is finalising: freeing device memory or destroying
# streams and events from a finaliser that runs during library unload is what crashed profiled runs at
# exit (rocprofv3 logs: SIGSEGV in __cxa_finalize).
_live = weakref.WeakSet()
_streams = []  # handles from h264mi_stream_create_cus not yet destroyed


def _close_all():
    for o in list(_live):
        try:
            o.close()
        except Exception:
            pass
    while _streams:
        h = _streams.pop()
        try:
            _hiprt().hipStreamSynchronize(ctypes.c_void_p(h))
            lib().h264mi_stream_destroy(ctypes.c_void_p(h))
        except Exception:
            pass


atexit.register(_close_all)


def _finalising():
    return sys.is_finalizing()


EXPORTED = ('init_encoder', 'force_key_frame', 'init_decoder', 'deinit_decoder', 'encode_frame',
            'encode_frame_yuv_i420', 'decode_frame_optimized', 'decode_frame_yuv_i420', 'free_buffer')


class Module:
    """Emscripten-``Module``-shaped facade over the C-ABI (the reference's JS glue surface).

    ``HEAPU8`` is a bytearray arena; ``_malloc`` returns offsets into it; ``cwrap`` returns callables
    that translate arena offsets to native pointers (and native output pointers back into arena
    offsets, e.g. the encoded buffer of encode_frame*), exactly as the workers expect
    (encoder_worker.js:163-187 reads the encoded buffer via getValue + HEAPU8.subarray).
    """

    def __init__(self, heap_bytes=64 << 20):
        self._L = lib()
        self.HEAPU8 = bytearray(heap_bytes)
        self._heap = (ctypes.c_ubyte * heap_bytes).from_buffer(self.HEAPU8)
        self._base = ctypes.addressof(self._heap)
        self._brk = 16
        self._freelist = {}  # offset -> size (first-fit)
        self._sizes = {}
        self._out_off, self._out_cap = 0, 0

    # -- heap management (Module._malloc / Module._free)
    def _malloc(self, n):
        n = (max(1, int(n)) + 15) & ~15
        for off, sz in sorted(self._freelist.items()):
            if sz >= n:
                del self._freelist[off]
                if sz > n:
                    self._freelist[off + n] = sz - n
                self._sizes[off] = n
                return off
        off = self._brk
        if off + n > len(self.HEAPU8):
            raise MemoryError('h264mi Module heap exhausted')
        self._brk += n
        self._sizes[off] = n
        return off

    def _free(self, off):
        n = self._sizes.pop(off, None)
        if n:
            self._freelist[off] = n

    def getValue(self, ptr, typ='i32'):
        assert typ == 'i32'
        return int.from_bytes(self.HEAPU8[ptr:ptr + 4], 'little', signed=True)

    def setValue(self, ptr, value, typ='i32'):
        assert typ == 'i32'
        self.HEAPU8[ptr:ptr + 4] = int(value).to_bytes(4, 'little', signed=True)

    def _p(self, off):
        return ctypes.c_void_p(self._base + off)

    def cwrap(self, name, ret, args):
        if name not in EXPORTED:
            raise KeyError(f'{name} is not exported by libh264mi')
        f = getattr(self._L, name)
        if name in ('encode_frame', 'encode_frame_yuv_i420'):
            def enc(src, w, h, out_pp, out_size_p, _f=f):
                native = ctypes.POINTER(ctypes.c_ubyte)()
                size = ctypes.c_int(0)
                _f(self._p(src), w, h, ctypes.byref(native), ctypes.byref(size))
                if size.value <= 0:
                    self.setValue(out_pp, 0)
                    self.setValue(out_size_p, 0)
                    return None
                if size.value > self._out_cap:  # library-owned output mirrored into the heap
                    if self._out_cap:
                        self._free(self._out_off)
                    self._out_off, self._out_cap = self._malloc(size.value), size.value
                ctypes.memmove(self._base + self._out_off, native, size.value)
                self.setValue(out_pp, self._out_off)
                self.setValue(out_size_p, size.value)
                return None
            return enc
        if name in ('decode_frame_optimized', 'decode_frame_yuv_i420'):
            def dec(idx, nal, size, out, w_p, h_p, _f=f):
                _f(idx, self._p(nal), size, self._p(out), self._p(w_p), self._p(h_p))
                return None
            return dec
        if name == 'free_buffer':
            return lambda ptr: None  # the reference glue never frees the library-owned buffer
        return lambda *a: f(*a)

    def on_runtime_initialized(self, cb):
        cb()


def slice_first_row(mbh, n, k):
    """first MB row of slice k of a picture of mbh MB rows coded as n slices (h264mi_slice_first_row; host only):
    (k * mbh) // n, mbh for k == n, -1 on bad arguments"""
    return lib().h264mi_slice_first_row(int(mbh), int(n), int(k))


class Quality(ctypes.Structure):
    """h264mi_quality (include/h264mi.h): one picture pair's distortion record, 64 bytes"""
    _fields_ = [('sse', ctypes.c_uint64 * 3), ('ssim_fix', ctypes.c_int64 * 3), ('windows', ctypes.c_uint32 * 2),
                ('coded', ctypes.c_uint32), ('reserved', ctypes.c_uint32)]

    def as_dict(self, w, h):
        """the record of a w x h pair as {'coded', 'sse', 'ssim_fix', 'windows', 'psnr', 'ssim'}; psnr (dB,
        h264mi_psnr) and ssim (the mean over the windows) per plane Y, Cb, Cr, None where nothing was coded"""
        coded = int(self.coded)
        samples = (w * h, (w // 2) * (h // 2), (w // 2) * (h // 2))
        win = (self.windows[0], self.windows[1], self.windows[1])
        sse, fix = [int(v) for v in self.sse], [int(v) for v in self.ssim_fix]
        return {'coded': coded, 'sse': sse, 'ssim_fix': fix, 'windows': [int(v) for v in self.windows],
                'psnr': [psnr(sse[p], samples[p]) for p in range(3)] if coded else None,
                'ssim': [fix[p] / (win[p] * 4294967296.0) for p in range(3)] if coded else None}


def psnr(sse, samples):
    """10 log10(255^2 samples / sse) in dB, 100.0 when sse == 0 (h264mi_psnr; host only)"""
    return lib().h264mi_psnr(int(sse), int(samples))


def _i420_bytes(w, h):
    """bytes of a tight w x h I420 frame"""
    return w * h + 2 * (w // 2) * (h // 2)


def _assert_dev_u8(*tensors):
    """these are contiguous uint8 device tensors"""
    import torch
    assert all(t.is_cuda and t.dtype == torch.uint8 for t in tensors)
    assert all(t.is_contiguous() for t in tensors)


def _hip_stream(stream):
    """HIP handle of stream, or of the current stream"""
    import torch
    return ctypes.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream)


def _byref(x):
    """x by reference, NULL for None"""
    return ctypes.byref(x) if x is not None else None


def _ptr(t):
    """tensor t's device pointer, NULL for None"""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class _Record(ctypes.Structure):
    """base of the parameter and record structures: the repr names every field (it appears in error messages)"""

    def __repr__(self):
        return type(self).__name__ + '(' + ', '.join(f'{k}={getattr(self, k)}' for k, _ in self._fields_) + ')'

    @classmethod
    def _of(cls, params):
        """None, an instance, or an instance from a tuple of integers"""
        if params is None or isinstance(params, cls):
            return params
        return cls(*(int(v) for v in params))


class BatchEncoder:
    """S independent encoder streams of one geometry, frames and NAL units resident in HBM."""

    def __init__(self, width, height, bitrate, nstreams, stream=None):
        self.w, self.h, self.S = width, height, nstreams
        self.frame_bytes = width * height * 3 // 2
        self.rgba_frame_bytes = width * height * 4
        self._L = lib()
        self._e = self._L.h264mi_enc_create(width, height, bitrate, nstreams, _hip_stream(stream))
        if not self._e:
            raise RuntimeError('h264mi_enc_create failed')
        self._ov_sprites = None  # the sprite tensor of the overlay list in force (set_overlays)
        _live.add(self)

    def encode(self, frames):
        """frames: uint8 CUDA tensor holding S tight I420 frames back to back (async)."""
        assert frames.is_cuda and frames.numel() >= self.S * self.frame_bytes
        if self._L.h264mi_enc_encode(self._e, ctypes.c_void_p(frames.data_ptr())) != 0:
            raise RuntimeError('h264mi_enc_encode failed')

    def encode_rgba(self, frames):
        """frames: uint8 CUDA tensor holding S tight RGBA8 frames (4 * w * h bytes each) back to back (async):
        one batched conversion on the encoder's stream, then the frame step of encode()"""
        assert frames.is_cuda and frames.numel() >= self.S * self.rgba_frame_bytes
        if self._L.h264mi_enc_encode_rgba(self._e, ctypes.c_void_p(frames.data_ptr())) != 0:
            raise RuntimeError('h264mi_enc_encode_rgba failed')

    def set_colorspec(self, spec):
        """what encode_rgba converts under from its next call on: a ColorSpec, or None for the default (BT.601 limited
        range, chroma of the top-left pixel: the bytes and the launch of before). No other input path changes.
        ValueError, with the previous specification still in force, on one colorspec_ok refuses."""
        if self._L.h264mi_enc_set_colorspec(self._e, _byref(spec)) != 0:
            raise ValueError(f'h264mi_enc_set_colorspec refused {spec!r}')

    def colorspec(self):
        """the specification in force (a copy)"""
        out = ColorSpec()
        if self._L.h264mi_enc_colorspec(self._e, ctypes.byref(out)) != 0:
            raise RuntimeError('h264mi_enc_colorspec failed')
        return out

    def encode_scaled(self, frames, src_w, src_h):
        """frames: uint8 CUDA tensor holding S tight I420 frames of src_w x src_h back to back, any alignment
        (async): one batched area-average downscale (i420_scale) into the encoder's input area on its stream, then
        the frame step of encode(); the quality records then compare the scaled source with the reconstruction.
        ValueError, with nothing enqueued, for a source smaller than the encoder, an odd size or one above 4096."""
        assert frames.is_cuda and frames.numel() >= self.S * _i420_bytes(src_w, src_h)
        if self._L.h264mi_enc_encode_scaled(self._e, ctypes.c_void_p(frames.data_ptr()), int(src_w), int(src_h)) != 0:
            raise ValueError(f'h264mi_enc_encode_scaled refused {src_w}x{src_h} -> {self.w}x{self.h}')

    def encode_oriented(self, frames, orient):
        """frames: uint8 CUDA tensor holding S tight I420 frames back to back, any alignment, of the size that orient
        (ORIENT_*) turns into the encoder's -- h x w for the four transposing orientations -- (async): one batched
        turn (i420_orient) into the encoder's input area on its stream, then an overlay list in force and the frame
        step of encode(); the quality records then compare the turned source with the reconstruction. ValueError,
        with nothing enqueued, for an unknown orientation, an encoder of odd size or frames inside the input area."""
        assert frames.is_cuda and frames.numel() >= self.S * _i420_bytes(self.w, self.h)
        if self._L.h264mi_enc_encode_oriented(self._e, ctypes.c_void_p(frames.data_ptr()), int(orient)) != 0:
            raise ValueError(f'h264mi_enc_encode_oriented refused orientation {orient} -> {self.w}x{self.h}')

    def encode_warped(self, frames, src_w, src_h, mesh, params, mesh_per_stream=False):
        """frames: uint8 CUDA tensor holding S tight I420 frames of src_w x src_h back to back, any alignment; mesh: int32
        CUDA tensor holding one mesh for the encoder's size, or S of them with mesh_per_stream; params: a Warp or
        (filter, edge, fill_y, fill_u, fill_v, grid_log2) (async): one batched warp (i420_warp) into the encoder's input
        area on its stream, then the stages in force and the frame step of encode(). ValueError, with nothing enqueued,
        for what i420_warp refuses, frames or a mesh inside the input area, or while the deinterlacer is on."""
        assert frames.is_cuda and frames.numel() >= self.S * _i420_bytes(src_w, src_h)
        d = Warp._of(params)
        _assert_dev_mesh(mesh, self.w, self.h, d, self.S if mesh_per_stream else 1)
        if self._L.h264mi_enc_encode_warped(self._e, _ptr(frames), int(src_w), int(src_h), _ptr(mesh), int(bool(mesh_per_stream)),
                                            _byref(d)) != 0:
            raise ValueError(f'h264mi_enc_encode_warped refused {src_w}x{src_h} -> {self.w}x{self.h}, {d!r}')

    def encode_pix(self, frames, layout):
        """frames: uint8 CUDA tensor holding S frames of the encoder's size in `layout` (a PixLayout: NV12, NV21, YUY2,
        UYVY or pitched I420; frame s at s * layout.frame_stride), any alignment (async): one batched conversion
        (pix_to_i420) into the encoder's input area on its stream, then an overlay list in force and the frame step
        of encode(). With pix_layout_tight(PIX_I420, w, h) the NAL bytes are those of encode(). ValueError, with
        nothing enqueued, for a layout that pix_layout_ok refuses for the encoder's size or frames inside the input area."""
        _assert_dev_u8(frames)
        assert pix_layout_ok(layout, self.w, self.h) != 0 or frames.numel() >= (self.S - 1) * layout.frame_stride + pix_span(layout, self.w, self.h)
        if self._L.h264mi_enc_encode_pix(self._e, ctypes.c_void_p(frames.data_ptr()), ctypes.byref(layout)) != 0:
            raise ValueError(f'h264mi_enc_encode_pix refused {layout!r} for {self.w}x{self.h}')

    def set_pixopt(self, opt):
        """the depth rule encode_pix converts the 10-bit layouts under from its next call on: a PixOpt, or None for the
        default (DEPTH_ROUND). ValueError, with the previous setting still in force, on one pixopt_ok refuses."""
        if self._L.h264mi_enc_set_pixopt(self._e, _byref(opt)) != 0:
            raise ValueError(f'h264mi_enc_set_pixopt refused {opt!r}')

    def pixopt(self):
        """the depth rule in force (a copy)"""
        out = PixOpt()
        if self._L.h264mi_enc_pixopt(self._e, ctypes.byref(out)) != 0:
            raise RuntimeError('h264mi_enc_pixopt failed')
        return out

    def encode_composed(self, src, src_w, src_h, nsrc, cells, bg=(16, 128, 128)):
        """src: uint8 CUDA tensor holding nsrc tight I420 frames of src_w x src_h back to back, any alignment; cells: a
        sequence of Cell whose canvases are this encoder's S input frames (async): with bg = (y, cb, cr) one fill of
        the whole input area, with bg=None none (uncovered samples keep what the input area held); then every cell's
        crop area-averaged into its rectangle (i420_compose), then the frame step of encode(), all on the encoder's
        stream. ValueError, with nothing enqueued, for whatever i420_compose refuses or a background above 255."""
        assert src.is_cuda and (nsrc <= 0 or min(src_w, src_h) <= 0 or src.numel() >= nsrc * _i420_bytes(src_w, src_h))
        arr = _cell_array(cells)
        y, cb, cr = (-1, 0, 0) if bg is None else (int(v) for v in bg)
        if self._L.h264mi_enc_encode_composed(self._e, ctypes.c_void_p(src.data_ptr()), int(src_w), int(src_h), int(nsrc), arr, len(arr),
                                              y, cb, cr) != 0:
            raise ValueError(f'h264mi_enc_encode_composed refused {len(arr)} cells of {nsrc} sources {src_w}x{src_h} -> {self.w}x{self.h}')

    def encode_composed_any(self, src, src_w, src_h, nsrc, cells, filter=1, bg=(16, 128, 128)):
        """encode_composed() with cells that may enlarge (i420_compose_any): a cell no larger than its crop is
        area-averaged as there, a cell at least as large both ways is enlarged with filter (FILTER_BILINEAR or
        FILTER_BICUBIC), taps clamped to the crop; then an overlay list in force and the frame step of encode(), all on
        the encoder's stream (h264mi_enc_encode_composed_any). ValueError, with nothing enqueued, for whatever
        i420_compose_any refuses or a background above 255."""
        assert src.is_cuda and (nsrc <= 0 or min(src_w, src_h) <= 0 or src.numel() >= nsrc * _i420_bytes(src_w, src_h))
        arr = _cell_array(cells)
        y, cb, cr = (-1, 0, 0) if bg is None else (int(v) for v in bg)
        if self._L.h264mi_enc_encode_composed_any(self._e, ctypes.c_void_p(src.data_ptr()), int(src_w), int(src_h), int(nsrc), arr, len(arr),
                                                  int(filter), y, cb, cr) != 0:
            raise ValueError(f'h264mi_enc_encode_composed_any refused {len(arr)} cells of {nsrc} sources {src_w}x{src_h} -> {self.w}x{self.h}')

    def _set_stage(self, name, cls, params):
        """h264mi_enc_set_<name> with what cls._of makes of params; ValueError when the library refuses"""
        d = cls._of(params)
        if getattr(self._L, 'h264mi_enc_set_' + name)(self._e, _byref(d)) != 0:
            raise ValueError(f'h264mi_enc_set_{name} refused {d!r}')

    def _get_stage(self, name, cls):
        """h264mi_enc_<name>: a cls (a copy) when the stage is on, None when it is off"""
        out = cls()
        r = getattr(self._L, 'h264mi_enc_' + name)(self._e, ctypes.byref(out))
        if r < 0:
            raise RuntimeError(f'h264mi_enc_{name} failed')
        return out if r == 1 else None

    def set_deinterlace(self, params):
        """the deinterlacer of encode(), encode_rgba() and encode_pix() from the next call on
        (h264mi_enc_set_deinterlace): a Deinterlace, a (parity, spatial, temporal, comb_level) tuple, or None for off. On,
        the encoder owns S frames of state -- the previous unfiltered input --, filters the input area in place in front
        of the denoiser, the key-frame policy and the overlay list, and rebuilds the first frame after it was turned on
        spatially only; encode() then codes a copy of the caller's frames, which stay as they are. While it is on
        encode_scaled, encode_composed, encode_composed_any and encode_oriented are refused. Off drops the state.
        ValueError, with the setting in force unchanged, on parameters deinterlace_ok refuses."""
        self._set_stage('deinterlace', Deinterlace, params)

    def deinterlace(self):
        """the deinterlacer in force: a Deinterlace (a copy), or None when it is off (h264mi_enc_deinterlace)"""
        return self._get_stage('deinterlace', Deinterlace)

    def set_denoise(self, params):
        """the pre-filter of every encode*() from its next call on (h264mi_enc_set_denoise): a Denoise, a
        (strength_y, strength_c, reach, motion) tuple, or None for off (both strengths 0 are off too). On, the encoder
        owns S frames of state -- the previous filtered frames --, filters the input area against them in front of
        the overlay list and the frame step, and codes the first frame after it was turned on unfiltered; encode() then
        codes a copy of the caller's frames, which stay as they are. Off drops the state. ValueError, with the setting
        in force unchanged, on parameters denoise_ok refuses."""
        self._set_stage('denoise', Denoise, params)

    def denoise(self):
        """the pre-filter in force: a Denoise (a copy), or None when it is off (h264mi_enc_denoise)"""
        return self._get_stage('denoise', Denoise)

    def set_levels(self, params):
        """the levels stage of every encode*() from its next call on (h264mi_enc_set_levels): a Levels, a (mode, clip_lo,
        clip_hi, in_lo, in_hi, out_lo, out_hi, max_gain, speed, sat) tuple, or None for off (a FIXED setting whose
        tables are the identity is off too). On, the encoder owns per stream 768 histogram words, 768 table bytes, 4
        state words and 8 record words and levels the input area in place behind the denoiser and in front of the
        spatial filter, the privacy masks, the key-frame policy and the overlay list; encode() then codes a copy of the
        caller's frames. The smoothed ends advance on every submitted frame; a change of the parameters keeps them, off
        drops them. ValueError, with the setting in force unchanged, on parameters levels_ok refuses."""
        self._set_stage('levels', Levels, params)

    def levels(self):
        """the levels setting in force: a Levels (a copy), or None when the stage is off (h264mi_enc_levels)"""
        return self._get_stage('levels', Levels)

    def levels_record(self):
        """the S streams' records of the last submitted frame (h264mi_enc_levels_record; waits for the encoder's
        stream): a list of S lists {lo_m, hi_m, lo_s, hi_s, lo_e, hi_e, below, above}. RuntimeError with the stage off."""
        out = (ctypes.c_int32 * (8 * self.S))()
        if self._L.h264mi_enc_levels_record(self._e, out, self.S) != 0:
            raise RuntimeError('h264mi_enc_levels_record failed')
        v = list(out)
        return [v[8 * s:8 * s + 8] for s in range(self.S)]

    def set_spatial(self, params):
        """the sharpen/blur filter of every encode*() from its next call on (h264mi_enc_set_spatial): a Spatial, a
        (radius_y, radius_c, amount_y, amount_c, core) tuple, or None for off (a setting that changes no plane is off
        too). On, the encoder owns S frames to filter into, behind the denoiser and in front of the privacy masks, the
        key-frame policy and the overlay list, which then work on those frames; encode_scaled() with the filter on is
        sharpen-after-downscale. Off frees the frames. ValueError, with the setting in force unchanged, on parameters
        spatial_ok refuses."""
        self._set_stage('spatial', Spatial, params)

    def spatial(self):
        """the spatial filter in force: a Spatial (a copy), or None when it is off (h264mi_enc_spatial)"""
        return self._get_stage('spatial', Spatial)

    def set_privacy(self, masks):
        """the privacy masks of every encode*() from its next call on (h264mi_enc_set_privacy): a sequence of Privacy
        whose `frame` is the stream index; an empty one (or None) clears the list. The masks are applied behind the
        spatial filter and in front of the key-frame policy and the overlay list: the samples never reach the stream,
        labels are blended over masks. ValueError, with the list in force unchanged, on a list privacy_ok refuses."""
        arr = _privacy_array(masks or ())
        if self._L.h264mi_enc_set_privacy(self._e, arr if len(arr) else None, len(arr)) != 0:
            raise ValueError(f'h264mi_enc_set_privacy refused {len(arr)} masks on {self.S} streams {self.w}x{self.h}')

    def privacy(self):
        """masks in force (h264mi_enc_privacy)"""
        return self._L.h264mi_enc_privacy(self._e)

    def set_scenecut(self, params):
        """the key-frame policy of every encode*() from its next call on (h264mi_enc_set_scenecut): a Scenecut, a
        (level, share, min_gap, max_gap, compensate) tuple, or None for off (share 0 with max_gap 0 is off too). On, the
        encoder owns a thumbnail and sixteen words per stream, runs the detector and a one-thread-per-stream decision
        behind the denoiser and in front of the overlay list and the frame step, and codes an IDR at a cut, at the
        period and whenever it would anyway; encode() then codes a copy of the caller's frames. Off drops the state.
        ValueError, with the setting in force unchanged, on parameters scenecut_ok refuses."""
        self._set_stage('scenecut', Scenecut, params)

    def scenecut(self):
        """the key-frame policy in force: a Scenecut (a copy), or None when it is off (h264mi_enc_scenecut)"""
        return self._get_stage('scenecut', Scenecut)

    def scenecut_state(self, stream):
        """stream's state after the last submitted frame (h264mi_enc_scenecut_state; waits for the encoder's stream): a
        dict of 'stats' (the frame's eight statistics words) and cut, key, reason, dist, keys_by_cut, keys_by_period,
        keys_other, frames"""
        out = (ctypes.c_uint32 * 16)()
        if self._L.h264mi_enc_scenecut_state(self._e, int(stream), out) != 0:
            raise RuntimeError('h264mi_enc_scenecut_state failed')
        v = list(out)
        return dict(zip(SCENECUT_STATE, v[8:]), stats=v[:8])

    def set_overlays(self, sprites, ow, oh, nsprites, overlays):
        """sprites: uint8 CUDA tensor holding nsprites I420A sprites of ow x oh back to back (i420a_bytes each), any
        alignment; overlays: a sequence of Overlay whose canvases are this encoder's S input frames. From the next
        frame step on every encode*() blends the list into the input area, in list order, in front of the frame step
        (h264mi_enc_set_overlays); encode() then codes a copy of the caller's frames, which stay as they are. The
        encoder keeps the placements and a reference to the tensor, whose bytes are read at every step. An empty
        sequence clears the list. ValueError, with the previous list still in force, for whatever i420_overlay
        refuses, a canvas the encoder has not, or sprites inside the input area."""
        arr = _overlay_array(overlays)
        if len(arr) == 0:
            return self.clear_overlays()
        assert sprites.is_cuda and (nsprites <= 0 or min(ow, oh) <= 0 or sprites.numel() >= nsprites * i420a_bytes(ow, oh))
        if self._L.h264mi_enc_set_overlays(self._e, ctypes.c_void_p(sprites.data_ptr()), int(ow), int(oh), int(nsprites), arr, len(arr)) != 0:
            raise ValueError(f'h264mi_enc_set_overlays refused {len(arr)} placements of {nsprites} sprites {ow}x{oh} on {self.w}x{self.h}')
        self._ov_sprites = sprites

    def clear_overlays(self):
        """no overlay list from the next frame step on: every encode*() enqueues what it did before one was set"""
        if self._L.h264mi_enc_set_overlays(self._e, None, 0, 0, 0, None, 0) != 0:
            raise RuntimeError('h264mi_enc_set_overlays failed')
        self._ov_sprites = None

    def overlays(self):
        """placements in force (h264mi_enc_overlays)"""
        return self._L.h264mi_enc_overlays(self._e)

    def force_idr(self, stream=-1):
        self._L.h264mi_enc_force_idr(self._e, stream)

    def set_frame_skip(self, on):
        """rate-control frame skipping (on by default, as the wrapper's encoder)"""
        if self._L.h264mi_enc_set_frame_skip(self._e, 1 if on else 0) != 0:
            raise RuntimeError('h264mi_enc_set_frame_skip failed')

    def inject_error(self, s=0, code=2):
        """test hook: stream s's next coded frame fails (0 bytes out, then an IDR)"""
        if self._L.h264mi_enc_inject_error(self._e, s, code) != 0:
            raise RuntimeError('h264mi_enc_inject_error failed')

    def set_gom_exact(self, on):
        """OpenH264's exact GOM rate control (h264mi_enc_set_gom_exact)"""
        if self._L.h264mi_enc_set_gom_exact(self._e, 1 if on else 0) != 0:
            raise RuntimeError('h264mi_enc_set_gom_exact failed')

    def set_slices(self, n):
        """every picture as n slices of whole MB rows from the next encode on (h264mi_enc_set_slices); ValueError on
        an n outside 1..min(MB rows, 32), or n > 1 with exact GOM rate control on"""
        if self._L.h264mi_enc_set_slices(self._e, int(n)) != 0:
            raise ValueError(f'h264mi_enc_set_slices({n}) refused')

    def slices(self):
        """slices per picture in force for the next encode (h264mi_enc_slices)"""
        return self._L.h264mi_enc_slices(self._e)

    def set_quality(self, on):
        """per-frame SSE / SSIM records of every stream from the next encode on (h264mi_enc_set_quality): one more
        launch per frame step, nothing else changes; ValueError for an encoder below 16x16"""
        if self._L.h264mi_enc_set_quality(self._e, 1 if on else 0) != 0:
            raise ValueError('h264mi_enc_set_quality refused')

    def quality_enabled(self):
        return self._L.h264mi_enc_quality_enabled(self._e) == 1

    def quality(self, s=0):
        """stream s's record of the last frame step (synchronises; h264mi_enc_quality) as a dict: 'sse' and
        'ssim_fix' (the exact integers), 'windows', 'coded' (0: the step coded nothing, all zeros), and per plane
        'psnr' (dB) and 'ssim' (mean), None when nothing was coded. RuntimeError while the option is off."""
        q = Quality()
        if self._L.h264mi_enc_quality(self._e, s, ctypes.byref(q)) != 0:
            raise RuntimeError('h264mi_enc_quality failed (set_quality(True) first)')
        return q.as_dict(self.w, self.h)

    def quality_ptr(self):
        """device address of the S records (h264mi_enc_quality_dev; 64 bytes each), None while the option is off"""
        return self._L.h264mi_enc_quality_dev(self._e)

    def gom_state(self, s=0):
        """exact GOM mode: the last P frame's per-GOM [QP, slice bits before it, target bits, last coded MB + 1]
        (h264mi_enc_gom_state)"""
        G = self._L.h264mi_enc_gom_state(self._e, s, None, 0)
        out = (ctypes.c_int * (4 * max(G, 1)))()
        if G < 0 or self._L.h264mi_enc_gom_state(self._e, s, out, 4 * G) != G:
            raise RuntimeError('h264mi_enc_gom_state failed')
        return [list(out[4 * g:4 * g + 4]) for g in range(G)]

    def frames_skipped(self, s=0):
        return self._L.h264mi_enc_frames_skipped(self._e, s)

    def rows_counter(self):
        """device address of the encoder's rows-started counter (h264mi_enc_rows_counter): S * mbh per frame step"""
        return self._L.h264mi_enc_rows_counter(self._e)

    def nal_sizes(self):
        out = (ctypes.c_int * self.S)()
        rc = self._L.h264mi_enc_nal_bytes(self._e, out)
        if rc != 0:
            raise RuntimeError(f'encoder kernels reported an error ({rc})')
        return list(out)

    def nal_ptr(self, s):
        return self._L.h264mi_enc_nal_ptr(self._e, s)

    def nal_ptrs(self):
        return [self.nal_ptr(s) for s in range(self.S)]

    def nal_bytes(self, s, size):
        """Copy stream s's last NAL output to host bytes (testing / C-ABI style use)."""
        import torch
        buf = torch.empty(size, dtype=torch.uint8)
        _hip_memcpy_d2h(buf.data_ptr(), self.nal_ptr(s), size)
        return bytes(buf.numpy())

    def nal_size_ptrs(self):
        return [self._L.h264mi_enc_nal_size_dev(self._e, s) for s in range(self.S)]

    def copy_nals(self, dst, slot, sizes=None):
        """async device copy of every stream's NAL into dst[s*slot:(s+1)*slot] (uint8 CUDA tensor);
        byte counts into sizes (int32 CUDA tensor of S) when given"""
        sp = _ptr(sizes)
        if self._L.h264mi_enc_copy_nals(self._e, ctypes.c_void_p(dst.data_ptr()), slot, sp) != 0:
            raise RuntimeError('h264mi_enc_copy_nals failed')

    def set_timing(self, on):
        self._L.h264mi_enc_set_timing(self._e, 1 if on else 0)

    def kernel_time(self):
        ms, n = ctypes.c_double(), ctypes.c_int()
        if self._L.h264mi_enc_kernel_time(self._e, ctypes.byref(ms), ctypes.byref(n)) != 0:
            raise RuntimeError('h264mi_enc_kernel_time failed')
        return ms.value, n.value

    def recon_ptr(self, s):
        return self._L.h264mi_enc_recon_ptr(self._e, s)

    def last_qp(self, s=0):
        return self._L.h264mi_enc_last_qp(self._e, s)

    RC_FIELDS = ('skipped', 'qp', 'avg_qp', 'target', 'remaining', 'fullness', 'continual', 'cmplx', 'min_qp',
                 'max_qp', 'bpf', 'pframes', 'idrs', 'skip_flag', 'remaining_weights', 'coded_in_vgop')

    def rc_state(self, s=0):
        """stream s's rate-control state after the last frame step (h264mi_enc_rc_state)"""
        out = (ctypes.c_int * 16)()
        if self._L.h264mi_enc_rc_state(self._e, s, out) != 0:
            raise RuntimeError('h264mi_enc_rc_state failed')
        return dict(zip(self.RC_FIELDS, list(out)))

    def close(self):
        if self._e:
            self._L.h264mi_enc_destroy(self._e)
            self._e = None

    def __del__(self):
        if _finalising():
            return
        try:
            self.close()
        except Exception:
            pass


def conceal_gaps(total_mbs, slices, max_gaps=33):
    """the gap rule of slice-copy concealment (h264mi_conceal_gaps; the decoder's kernels call the same function):
    slices = [(first_mb, end_mb, ok), ...] of one picture in any order -> [(first, end, donor index), ...] in address
    order ([] for an exact tiling), or None when the picture is rejected (no good slice, an overlap, a bad argument)"""
    n = len(slices)
    arr = [(ctypes.c_int * max(1, n))(*[int(sl[k]) for sl in slices]) for k in range(3)]
    out = (ctypes.c_int * (3 * max(1, max_gaps)))()
    r = lib().h264mi_conceal_gaps(total_mbs, n, arr[0], arr[1], arr[2], out, max_gaps)
    if r < 0:
        return None
    return [(out[3 * g], out[3 * g + 1], out[3 * g + 2]) for g in range(min(r, max_gaps))]


def masked_stream(cu_lo, cu_hi, complement=False):
    """A torch stream (ExternalStream over h264mi_stream_create_cus) restricted to CU mask bits
    [cu_lo, cu_hi), or to every other CU. Pairs with BatchDecoder.set_parse_cus."""
    import torch
    h = lib().h264mi_stream_create_cus(cu_lo, cu_hi, 1 if complement else 0)
    if not h:
        raise RuntimeError('h264mi_stream_create_cus failed')
    _streams.append(h)
    return torch.cuda.ExternalStream(h)


def destroy_stream(st):
    """Synchronise and destroy a stream made by masked_stream() (close its users first)."""
    h = st.cuda_stream
    if h in _streams:
        _streams.remove(h)
        st.synchronize()
        lib().h264mi_stream_destroy(ctypes.c_void_p(h))


class BatchDecoder:
    """S independent decoder streams of one geometry; NAL units in HBM. max_frames > 1 enables
    decode_frames(): several access units per stream per call, entropy-decoded concurrently."""

    def __init__(self, width, height, nstreams, stream=None, max_frames=1, groups=0, parse_streams=3):
        """groups: slot groups of max_frames frames in the decoder's ring (0 = default, up to 16; 2 for a
        caller that waits for every call); parse_streams: HIP streams entropy decoding rotates over"""
        self.w, self.h, self.S, self.B = width, height, nstreams, max_frames
        self._L = lib()
        self._d = self._L.h264mi_dec_create_ring(width, height, nstreams, max_frames, groups, parse_streams, _hip_stream(stream))
        if not self._d:
            raise RuntimeError('h264mi_dec_create failed')
        _live.add(self)
        cw, ch = ctypes.c_int(), ctypes.c_int()
        self._L.h264mi_dec_coded_size(self._d, ctypes.byref(cw), ctypes.byref(ch))
        self.cw, self.ch = cw.value, ch.value

    def decode(self, nal_ptrs, nal_sizes):
        """nal_ptrs: device addresses (ints); nal_sizes: host ints (async)."""
        ptrs = (ctypes.c_void_p * self.S)(*nal_ptrs)
        sizes = (ctypes.c_int * self.S)(*nal_sizes)
        if self._L.h264mi_dec_decode(self._d, ptrs, sizes) != 0:
            raise RuntimeError('h264mi_dec_decode failed')

    def decode_dev(self, nal_ptrs, size_ptrs):
        """async; sizes read on the device from size_ptrs (e.g. BatchEncoder.nal_size_ptrs())"""
        ptrs = (ctypes.c_void_p * self.S)(*nal_ptrs)
        sz = (ctypes.c_void_p * self.S)(*size_ptrs)
        if self._L.h264mi_dec_decode_dev(self._d, ptrs, sz) != 0:
            raise RuntimeError('h264mi_dec_decode_dev failed')

    def decode_frames(self, nal_ptrs, nal_sizes=None, size_ptrs=None, ready_event=None, out_ptrs=None, got_ptrs=None):
        """async; n frames per stream: nal_ptrs[f * S + s] (device addresses), sizes either host ints
        (nal_sizes) or device int32 addresses (size_ptrs). n <= max_frames. Inputs are ordered after
        the decoder's stream, or, if ready_event (a torch.cuda.Event recorded by the producer, or a
        list of them, one per producer stream) is given, after those events only. out_ptrs / got_ptrs
        (device addresses, same indexing): every frame's cropped picture and got flag. An out buffer holds
        w * h * 3 // 2 bytes (tight I420) with the output format 'i420', w * h * 4 bytes (tight RGBA8, 4-byte
        aligned) with 'rgba' (set_output_format), pix_span(layout, w, h) bytes with a layout (set_output_layout); it
        is left untouched when got is 0."""
        m = len(nal_ptrs)
        assert m % self.S == 0 and m // self.S <= self.B
        ptrs = (ctypes.c_void_p * m)(*nal_ptrs)
        sizes = (ctypes.c_int * m)(*nal_sizes) if nal_sizes is not None else None
        sp = (ctypes.c_void_p * m)(*size_ptrs) if size_ptrs is not None else None
        evs = [] if ready_event is None else (list(ready_event) if isinstance(ready_event, (list, tuple)) else [ready_event])
        ev = (ctypes.c_void_p * max(1, len(evs)))(*[e.cuda_event for e in evs])
        op = (ctypes.c_void_p * m)(*out_ptrs) if out_ptrs is not None else None
        gp = (ctypes.c_void_p * m)(*got_ptrs) if got_ptrs is not None else None
        if self._L.h264mi_dec_decode_frames_out(self._d, m // self.S, ptrs, sizes, sp, ev, len(evs), op, gp) != 0:
            raise RuntimeError('h264mi_dec_decode_frames failed')

    OUTPUT_FORMATS = {'i420': 0, 'rgba': 1}  # H264MI_FMT_*

    def set_output_format(self, fmt):
        """what decode_frames writes to out_ptrs from the next call on: 'i420' (default) or 'rgba'"""
        if fmt not in self.OUTPUT_FORMATS or self._L.h264mi_dec_set_output_format(self._d, self.OUTPUT_FORMATS[fmt]) != 0:
            raise ValueError(f'h264mi_dec_set_output_format({fmt!r}) refused')

    def output_format(self):
        """'i420', 'rgba', or 'layout' while a layout is in effect (set_output_layout)"""
        fmt = self._L.h264mi_dec_output_format(self._d)
        return 'layout' if fmt == FMT_LAYOUT else {v: k for k, v in self.OUTPUT_FORMATS.items()}[fmt]

    def set_output_layout(self, layout):
        """what decode_frames writes to out_ptrs from the next call on: every frame's cropped picture in `layout` (a
        PixLayout checked against the decoder's width x height; frame_stride is unused, every out pointer is a frame's
        base and must hold pix_span(layout, w, h) bytes), or None: back to the format set last. The last setter
        wins: set_output_format clears a layout. ValueError, with nothing changed, on a layout pix_layout_ok refuses."""
        if self._L.h264mi_dec_set_output_layout(self._d, _byref(layout)) != 0:
            raise ValueError(f'h264mi_dec_set_output_layout refused {layout!r} for {self.w}x{self.h}')

    def output_layout(self):
        """the layout in effect (a copy), or None"""
        out = PixLayout()
        return out if self._L.h264mi_dec_output_layout(self._d, ctypes.byref(out)) == 1 else None

    def set_output_colorspec(self, spec):
        """what 'rgba' output converts under from the next decode_frames call on (each call captures its setting): a
        ColorSpec, or None for the default (BT.601 limited range, chroma repeated: the bytes and the launch of before).
        Nothing changes for 'i420' or layout output; the setting is kept across format changes. BILINEAR clamps to the
        cropped picture: the bytes equal i420_to_rgba(..., spec=spec) on the cropped I420 picture. ValueError, with
        nothing changed, on one colorspec_ok refuses."""
        if self._L.h264mi_dec_set_output_colorspec(self._d, _byref(spec)) != 0:
            raise ValueError(f'h264mi_dec_set_output_colorspec refused {spec!r}')

    def output_colorspec(self):
        """the specification in force (a copy)"""
        out = ColorSpec()
        if self._L.h264mi_dec_output_colorspec(self._d, ctypes.byref(out)) != 0:
            raise RuntimeError('h264mi_dec_output_colorspec failed')
        return out

    def set_parse_cus(self, lo, hi):
        """entropy decoding on CU mask bits [lo, hi) (see h264mi_dec_set_parse_cus)"""
        if self._L.h264mi_dec_set_parse_cus(self._d, lo, hi) != 0:
            raise RuntimeError('h264mi_dec_set_parse_cus failed')

    def set_recon_gate(self, counter, target, step, count, limit_us=4000):
        """for the next decode call: frame f < count reconstructs once the device uint32 at `counter` reaches
        target + f * step (h264mi_dec_set_recon_gate; a scheduling hint, bounded by limit_us)"""
        if self._L.h264mi_dec_set_recon_gate(self._d, counter, target & 0xffffffff, step & 0xffffffff, count, limit_us) != 0:
            raise RuntimeError('h264mi_dec_set_recon_gate failed')

    def set_streamed(self, mode):
        """streamed reconstruction (h264mi_dec_set_streamed): 1 on (the reconstruction stream is kept off the
        parse CUs), 0 off, -1 automatic"""
        if self._L.h264mi_dec_set_streamed(self._d, mode) != 0:
            raise RuntimeError('h264mi_dec_set_streamed failed')

    def streamed(self):
        return self._L.h264mi_dec_streamed(self._d)

    def set_resolve(self, mode):
        """record resolution ahead of the reconstruction (h264mi_dec_set_resolve): 1 on the parse stream (default),
        0 inside the reconstruction (what a streamed call always does)"""
        if self._L.h264mi_dec_set_resolve(self._d, mode) != 0:
            raise RuntimeError('h264mi_dec_set_resolve failed')

    def resolve_launches(self):
        return self._L.h264mi_dec_resolve_launches(self._d)

    def set_conceal(self, mode):
        """slice-copy concealment of lost slices (h264mi_dec_set_conceal): 1 on, 0 off (default). While it is on no call
        is streamed. ValueError, with nothing changed, on any other mode."""
        if self._L.h264mi_dec_set_conceal(self._d, mode) != 0:
            raise ValueError(f'h264mi_dec_set_conceal({mode!r}) refused')

    def conceal(self):
        return self._L.h264mi_dec_conceal(self._d)

    def concealed(self):
        """synchronises; per frame of the last decode call, the macroblocks concealed in each stream: [[mbs] * S] * frames"""
        out = (ctypes.c_int * (self.S * self.B))()
        n = self._L.h264mi_dec_concealed(self._d, out)
        if n < 0:
            raise RuntimeError('h264mi_dec_concealed failed')
        return [list(out[f * self.S:(f + 1) * self.S]) for f in range(n)]

    def concealed_ptr(self):
        """device address of the same table (max_frames x S int32), written in stream order"""
        return self._L.h264mi_dec_concealed_ptr(self._d)

    def set_slice_waves(self, k):
        """slice-data waves per picture (h264mi_dec_set_slice_waves): a multi-slice picture's slices in parallel"""
        if self._L.h264mi_dec_set_slice_waves(self._d, k) != 0:
            raise RuntimeError('h264mi_dec_set_slice_waves failed')

    def set_parse_streams(self, n):
        if self._L.h264mi_dec_set_parse_streams(self._d, n) != 0:
            raise RuntimeError('h264mi_dec_set_parse_streams failed')

    def set_timing(self, on):
        self._L.h264mi_dec_set_timing(self._d, 1 if on else 0)

    def kernel_time(self, which=0):
        """(total ms, launches) of dec_recon_kernel (which 0) or dec_parse_kernel (1) since set_timing"""
        ms, n = ctypes.c_double(), ctypes.c_int()
        if self._L.h264mi_dec_kernel_time(self._d, which, ctypes.byref(ms), ctypes.byref(n)) != 0:
            raise RuntimeError('h264mi_dec_kernel_time failed')
        return ms.value, n.value

    def device_bytes(self):
        return self._L.h264mi_dec_device_bytes(self._d)

    def ring_groups(self):
        return self._L.h264mi_dec_ring_groups(self._d)

    def status(self):
        got = (ctypes.c_int * self.S)()
        rc = self._L.h264mi_dec_status(self._d, got)
        return rc, list(got)

    def picture_ptr(self, s):
        """Device pointer of stream s's last decoded picture (coded size, planes contiguous)."""
        return self._L.h264mi_dec_picture_ptr(self._d, s)

    def picture_i420(self, s):
        """Cropped tight I420 of stream s's last picture, as host bytes."""
        import numpy as np
        p = self._L.h264mi_dec_picture_ptr(self._d, s)
        cw, ch = self.cw, self.ch
        buf = np.empty(cw * ch * 3 // 2, np.uint8)
        _hip_memcpy_d2h(buf.ctypes.data, p, buf.size)  # planes are contiguous: Y, U, V at coded size
        y = buf[:cw * ch].reshape(ch, cw)[:self.h, :self.w]
        u = buf[cw * ch:cw * ch * 5 // 4].reshape(ch // 2, cw // 2)[:self.h // 2, :self.w // 2]
        v = buf[cw * ch * 5 // 4:].reshape(ch // 2, cw // 2)[:self.h // 2, :self.w // 2]
        return np.concatenate([y.ravel(), u.ravel(), v.ravel()]).tobytes()

    def close(self):
        if self._d:
            self._L.h264mi_dec_destroy(self._d)
            self._d = None

    def __del__(self):
        if _finalising():
            return
        try:
            self.close()
        except Exception:
            pass


class NalRing:
    """Device-resident NAL ring: the reference's SharedArrayBuffer frame pool (app.js:52-53,
    :292-310) with encoder_worker.js:163-202 publish and decoder_worker.js:138-164 release semantics,
    decided on the device. Tickets are returned by publish(); decoders read nal_ptr(t)/size_ptr(t)
    (size 0 = dropped, decoders skip it) and every consumer calls release(t) afterwards."""

    def __init__(self, slots=40, slot_bytes=2 << 20):
        self._L = lib()
        self.slots, self.slot_bytes = slots, slot_bytes
        self._r = self._L.h264mi_ring_create(slots, slot_bytes)
        if not self._r:
            raise RuntimeError('h264mi_ring_create failed')
        _live.add(self)

    def publish(self, enc, stream, consumers):
        t = self._L.h264mi_ring_publish(self._r, enc._e, stream, consumers)
        if t < 0:
            raise RuntimeError(f'h264mi_ring_publish failed ({t})')
        return t

    def nal_ptr(self, t):
        return self._L.h264mi_ring_nal_ptr(self._r, t)

    def size_ptr(self, t):
        return self._L.h264mi_ring_size_dev(self._r, t)

    def release(self, t, stream=None):
        if self._L.h264mi_ring_release(self._r, t, _hip_stream(stream)) != 0:
            raise RuntimeError('h264mi_ring_release failed')

    def stats(self):
        p, b, z = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        refs = (ctypes.c_int * self.slots)()
        if self._L.h264mi_ring_stats(self._r, ctypes.byref(p), ctypes.byref(b), ctypes.byref(z), refs) != 0:
            raise RuntimeError('h264mi_ring_stats failed')
        return {'published': p.value, 'dropped_busy': b.value, 'dropped_size': z.value, 'ref_counts': list(refs)}

    def close(self):
        if self._r:
            self._L.h264mi_ring_destroy(self._r)
            self._r = None

    def __del__(self):
        if _finalising():
            return
        try:
            self.close()
        except Exception:
            pass


def _hip_memcpy_d2h(dst, src, n):
    import torch
    t = torch.cuda.current_stream()
    t.synchronize()
    hip = _hiprt()
    rc = hip.hipMemcpy(ctypes.c_void_p(dst), ctypes.c_void_p(src), ctypes.c_size_t(n), 2)
    if rc != 0:
        raise RuntimeError(f'hipMemcpy failed ({rc})')


_hip = None


def _hiprt():
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL('libamdhip64.so')
        _hip.hipMemcpy.restype = ctypes.c_int
        _hip.hipStreamSynchronize.restype = ctypes.c_int
        _hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    return _hip


def _convert_dev(fn, dst, src, dst_bytes, src_bytes, w, h, n, stream):
    _assert_dev_u8(dst, src)
    assert n <= 0 or (dst.numel() >= n * dst_bytes and src.numel() >= n * src_bytes)
    if fn(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()), w, h, n, _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {w}x{h}, {n} frames')


MATRIX_BT601, MATRIX_BT709 = 0, 1                # H264MI_MATRIX_*
RANGE_LIMITED, RANGE_FULL = 0, 1                 # H264MI_RANGE_*: Y 16..235 and Cb/Cr 16..240, or 0..255
CHROMA_DOWN_TOPLEFT, CHROMA_DOWN_AVERAGE = 0, 1  # H264MI_CHROMA_DOWN_*: RGBA -> 4:2:0 from the top-left pixel of each 2x2, or from the sum of the four
CHROMA_UP_REPEAT, CHROMA_UP_BILINEAR = 0, 1      # H264MI_CHROMA_UP_*: 4:2:0 -> RGBA by repetition, or centre-sited 9-3-3-1 interpolation


class ColorSpec(_Record):
    """h264mi_colorspec (include/h264mi.h): the matrix, the range and how chroma is reduced and restored at an RGBA
    edge; all 0 is the reference wrapper's conversion. 16 bytes"""
    _fields_ = [(k, ctypes.c_int32) for k in ('matrix', 'range', 'chroma_down', 'chroma_up')]


def colorspec_ok(spec):
    """0 when every field of spec is 0 or 1, else -1 (None included); h264mi_colorspec_ok, host only"""
    return lib().h264mi_colorspec_ok(_byref(spec))


def _convert_cs_dev(fn, dst, src, dst_bytes, src_bytes, w, h, n, spec, stream):
    _assert_dev_u8(dst, src)
    assert n <= 0 or min(w, h) <= 0 or (dst.numel() >= n * dst_bytes and src.numel() >= n * src_bytes)
    if fn(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()), w, h, n, ctypes.byref(spec), _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {w}x{h}, {n} frames, {spec!r}')


def rgba_to_i420(dst, src, w, h, n, stream=None, spec=None):
    """n tight RGBA8 frames (uint8 CUDA tensor src) to n tight I420 frames (dst), one launch, async on stream
    (default: the current one); h264mi_rgba_to_i420_dev, or with spec (a ColorSpec) h264mi_rgba_to_i420_cs_dev: its
    matrix, range and chroma_down; the bytes equal tests/csref.py's. That call also refuses (ValueError) a side outside
    2..8192 and overlapping buffers."""
    if spec is None:
        return _convert_dev(lib().h264mi_rgba_to_i420_dev, dst, src, w * h * 3 // 2, w * h * 4, w, h, n, stream)
    _convert_cs_dev(lib().h264mi_rgba_to_i420_cs_dev, dst, src, w * h * 3 // 2, w * h * 4, w, h, n, spec, stream)


def i420_to_rgba(dst, src, w, h, n, stream=None, spec=None):
    """n tight I420 frames (uint8 CUDA tensor src) to n tight RGBA8 frames (dst, A = 255); h264mi_i420_to_rgba_dev, or
    with spec (a ColorSpec) h264mi_i420_to_rgba_cs_dev: its matrix, range and chroma_up; ValueError as rgba_to_i420"""
    if spec is None:
        return _convert_dev(lib().h264mi_i420_to_rgba_dev, dst, src, w * h * 4, w * h * 3 // 2, w, h, n, stream)
    _convert_cs_dev(lib().h264mi_i420_to_rgba_cs_dev, dst, src, w * h * 4, w * h * 3 // 2, w, h, n, spec, stream)


def i420_scale(dst, src, sw, sh, dw, dh, n, stream=None):
    """n tight sw x sh I420 frames (uint8 CUDA tensor src, any alignment) area-averaged down to n tight dw x dh
    frames (dst), one launch, async on stream (default: the current one); h264mi_i420_scale_dev. Exact integers:
    the bytes equal tests/scaleref.py's. ValueError on a bad argument (odd sizes, dw > sw, dh > sh, a source above
    4096, n <= 0, overlapping buffers)."""
    _assert_dev_u8(dst, src)
    assert n <= 0 or min(sw, sh, dw, dh) <= 0 or (dst.numel() >= n * _i420_bytes(dw, dh) and src.numel() >= n * _i420_bytes(sw, sh))
    if lib().h264mi_i420_scale_dev(ctypes.c_void_p(dst.data_ptr()), dw, dh, ctypes.c_void_p(src.data_ptr()), sw, sh, n,
                                   _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {sw}x{sh} -> {dw}x{dh}, {n} frames')


class Cell(_Record):
    """h264mi_cell (include/h264mi.h): a crop (sx, sy, sw, sh) of source frame src to a rectangle (dx, dy, dw, dh) of
    canvas `canvas`, 40 bytes"""
    _fields_ = [(k, ctypes.c_int32) for k in ('src', 'canvas', 'sx', 'sy', 'sw', 'sh', 'dx', 'dy', 'dw', 'dh')]


def _cell_array(cells):
    cells = list(cells)
    return (Cell * len(cells))(*cells)


def mosaic_cells(n, src_w, src_h, cw, ch):
    """the gallery layout of n whole src_w x src_h sources on canvas 0 of cw x ch as a list of Cell
    (h264mi_mosaic_cells; host only): the smallest square grid that holds n, every picture as large as its slot allows
    at the source's shape, never enlarged, centred. ValueError on a bad argument or a cell below 2 samples."""
    arr = (Cell * max(int(n), 1))()
    if lib().h264mi_mosaic_cells(arr, len(arr), int(n), int(src_w), int(src_h), int(cw), int(ch)) != n:
        raise ValueError(f'bad arguments: {n} sources {src_w}x{src_h} on {cw}x{ch}')
    return list(arr)


def i420_compose(canvas, cw, ch, ncanvas, src, src_w, src_h, nsrc, cells, stream=None):
    """every cell's crop of one of nsrc tight src_w x src_h I420 frames (uint8 CUDA tensor src) area-averaged into its
    rectangle of one of ncanvas tight cw x ch I420 frames (canvas), any alignment, async on stream (default: the
    current one); h264mi_i420_compose_dev. Canvas bytes outside the rectangles keep their value. Exact integers: the
    bytes equal tests/composeref.py's. ValueError on a bad argument (odd fields, a crop outside the source, a rectangle
    outside the canvas or larger than its crop, overlapping cells of one canvas, overlapping buffers, more than 4096
    cells)."""
    _assert_dev_u8(canvas, src)
    assert min(ncanvas, nsrc, src_w, src_h, cw, ch) <= 0 or (canvas.numel() >= ncanvas * _i420_bytes(cw, ch) and
                                                             src.numel() >= nsrc * _i420_bytes(src_w, src_h))
    arr = _cell_array(cells)
    if lib().h264mi_i420_compose_dev(ctypes.c_void_p(canvas.data_ptr()), cw, ch, ncanvas, ctypes.c_void_p(src.data_ptr()), src_w, src_h,
                                     nsrc, arr, len(arr), _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {len(arr)} cells of {nsrc} sources {src_w}x{src_h} on {ncanvas} canvases {cw}x{ch}')


FILTER_BILINEAR = 0  # H264MI_FILTER_BILINEAR
FILTER_BICUBIC = 1   # H264MI_FILTER_BICUBIC (Catmull-Rom)


def i420_upscale(dst, src, sw, sh, dw, dh, n, filter=FILTER_BICUBIC, stream=None):
    """n tight sw x sh I420 frames (uint8 CUDA tensor src, any alignment) enlarged to n tight dw x dh frames (dst) with
    FILTER_BILINEAR or FILTER_BICUBIC, async on stream (default: the current one); h264mi_i420_upscale_dev. Exact
    integers: the bytes equal tests/upscaleref.py's; equal sizes copy. ValueError on a bad argument (odd sizes, dw < sw,
    dh < sh, a source above 4096, a destination above 8192, an unknown filter, n <= 0, overlapping buffers)."""
    _assert_dev_u8(dst, src)
    assert n <= 0 or min(sw, sh, dw, dh) <= 0 or (dst.numel() >= n * _i420_bytes(dw, dh) and src.numel() >= n * _i420_bytes(sw, sh))
    if lib().h264mi_i420_upscale_dev(ctypes.c_void_p(dst.data_ptr()), dw, dh, ctypes.c_void_p(src.data_ptr()), sw, sh, n, int(filter),
                                     _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {sw}x{sh} -> {dw}x{dh}, {n} frames, filter {filter}')


def speaker_cells(n, speaker, src_w, src_h, cw, ch):
    """the active-speaker layout of n whole src_w x src_h sources on canvas 0 of cw x ch as a list of Cell
    (h264mi_speaker_cells; host only): source `speaker` above a strip of the others an eighth of the canvas high, every
    picture as large as its slot allows at the source's shape, enlarged where the slot is larger, centred. ValueError
    on a bad argument or a cell below 2 samples."""
    arr = (Cell * max(int(n), 1))()
    if lib().h264mi_speaker_cells(arr, len(arr), int(n), int(speaker), int(src_w), int(src_h), int(cw), int(ch)) != n:
        raise ValueError(f'bad arguments: {n} sources {src_w}x{src_h} on {cw}x{ch}, speaker {speaker}')
    return list(arr)


def i420_compose_any(canvas, cw, ch, ncanvas, src, src_w, src_h, nsrc, cells, filter=FILTER_BICUBIC, stream=None):
    """i420_compose() with cells that may enlarge (h264mi_i420_compose_any_dev): a cell no larger than its crop gets
    i420_compose's bytes, a cell at least as large both ways is enlarged with filter as i420_upscale does, taps clamped
    to the crop. Exact integers: the bytes equal tests/upscaleref.py's. ValueError on whatever i420_compose refuses but
    a rectangle larger than its crop, on a cell that enlarges one axis and shrinks the other, and on an unknown
    filter."""
    _assert_dev_u8(canvas, src)
    assert min(ncanvas, nsrc, src_w, src_h, cw, ch) <= 0 or (canvas.numel() >= ncanvas * _i420_bytes(cw, ch) and
                                                             src.numel() >= nsrc * _i420_bytes(src_w, src_h))
    arr = _cell_array(cells)
    if lib().h264mi_i420_compose_any_dev(ctypes.c_void_p(canvas.data_ptr()), cw, ch, ncanvas, ctypes.c_void_p(src.data_ptr()), src_w, src_h,
                                         nsrc, arr, len(arr), int(filter), _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {len(arr)} cells of {nsrc} sources {src_w}x{src_h} on {ncanvas} canvases {cw}x{ch}, filter {filter}')


ORIENT_IDENTITY = 0    # H264MI_ORIENT_*: D[y][x] = S[y][x]
ORIENT_ROT90 = 1       # a quarter turn clockwise, S[ph-1-x][y]
ORIENT_ROT180 = 2      # S[ph-1-y][pw-1-x]
ORIENT_ROT270 = 3      # three quarter turns clockwise, S[x][pw-1-y]
ORIENT_MIRROR = 4      # left-right, S[y][pw-1-x]
ORIENT_FLIP = 5        # top-bottom, S[ph-1-y][x]
ORIENT_TRANSPOSE = 6   # S[x][y]
ORIENT_TRANSVERSE = 7  # S[ph-1-x][pw-1-y]


def orient_size(orient, w, h):
    """(width, height) of a w x h frame turned by orient (h264mi_orient_size; host only): (h, w) for ROT90, ROT270,
    TRANSPOSE and TRANSVERSE. ValueError on an unknown orientation or a side that is odd or outside 2..8192."""
    dw, dh = ctypes.c_int(), ctypes.c_int()
    if lib().h264mi_orient_size(int(orient), int(w), int(h), ctypes.byref(dw), ctypes.byref(dh)) != 0:
        raise ValueError(f'bad arguments: orientation {orient} of {w}x{h}')
    return dw.value, dh.value


def orient_compose(first, then):
    """the one orientation that equals turning by `first`, then by `then` (h264mi_orient_compose; host only)"""
    r = lib().h264mi_orient_compose(int(first), int(then))
    if r < 0:
        raise ValueError(f'bad orientations: {first}, {then}')
    return r


def orient_inverse(orient):
    """the orientation that undoes orient (h264mi_orient_inverse; host only)"""
    r = lib().h264mi_orient_inverse(int(orient))
    if r < 0:
        raise ValueError(f'bad orientation: {orient}')
    return r


def i420_orient(dst, src, sw, sh, n, orient, stream=None):
    """n tight sw x sh I420 frames (uint8 CUDA tensor src, any alignment) turned by orient (ORIENT_*) into n tight frames
    of orient_size(orient, sw, sh) (dst, the same byte count), every plane on its own, one launch, async on stream
    (default: the current one); h264mi_i420_orient_dev. Samples are moved, never interpolated: the bytes equal
    tests/orientref.py's. ValueError on a bad argument (an unknown orientation, a side that is odd or outside 2..8192,
    n <= 0, overlapping buffers)."""
    _assert_dev_u8(dst, src)
    assert n <= 0 or min(sw, sh) <= 0 or min(dst.numel(), src.numel()) >= n * _i420_bytes(sw, sh)
    if lib().h264mi_i420_orient_dev(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()), sw, sh, n, int(orient),
                                    _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: orientation {orient} of {n} frames {sw}x{sh}')


class Denoise(_Record):
    """h264mi_denoise (include/h264mi.h): strength_y, strength_c 0..224 (the share of 256 of a vanishing difference that
    is removed), reach 1..32 (differences of reach or more are kept), motion 0..1020 (the mean absolute luma difference
    of an 8x8 block, in quarter levels, above which the block is left as it is). 16 bytes"""
    _fields_ = [(k, ctypes.c_int32) for k in ('strength_y', 'strength_c', 'reach', 'motion')]


def denoise_ok(params):
    """0 when every field of params (a Denoise or four integers) is in its range, else -1 (None included);
    h264mi_denoise_ok, host only"""
    return lib().h264mi_denoise_ok(_byref(Denoise._of(params)))


def i420_denoise(dst, cur, prev, w, h, n, params, dst2=None, stats=None, stream=None):
    """n tight w x h I420 frames (uint8 CUDA tensor cur, any alignment) filtered against the n previous filtered frames
    (prev) into dst and, when given, the same bytes into dst2; one launch, async on stream (default: the current one);
    h264mi_i420_denoise_dev. params: a Denoise or (strength_y, strength_c, reach, motion). stats, when given: a CUDA
    tensor of 4 n 32-bit words, per frame {moving blocks, blocks, sum of m over luma, over both chroma planes}, zeroed
    and then accumulated on the stream. dst and dst2 may each be exactly cur or exactly prev. The bytes equal
    tests/denoiseref.py's. ValueError on a bad argument (a parameter out of range, a side that is odd or outside
    2..8192, n < 1, any other overlap)."""
    _assert_dev_u8(dst, cur, prev)
    if dst2 is not None:
        _assert_dev_u8(dst2)
    need = 0 if n <= 0 or min(w, h) <= 0 else n * _i420_bytes(w, h)
    assert all(t.numel() >= need for t in (dst, cur, prev) + ((dst2,) if dst2 is not None else ()))
    if stats is not None:
        assert stats.is_cuda and stats.is_contiguous() and stats.numel() * stats.element_size() >= 16 * max(n, 0)
    d = Denoise._of(params)
    if lib().h264mi_i420_denoise_dev(_ptr(dst), _ptr(dst2), _ptr(cur), _ptr(prev), w, h, n, _byref(d), _ptr(stats),
                                     _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {n} frames {w}x{h}, {d!r}')


class Scenecut(_Record):
    """h264mi_scenecut (include/h264mi.h): level 0..1020 (the mean absolute thumbnail difference of a 32x32 block, in
    quarter levels, above which the block is changed), share 0..256 (the share of 256 of the blocks that must be
    changed; 0: detection off), min_gap, max_gap 0..65535 (frames between key frames; max_gap 0: no period),
    compensate 0/1 (a uniform brightness step changes no block). 20 bytes"""
    _fields_ = [(k, ctypes.c_int32) for k in ('level', 'share', 'min_gap', 'max_gap', 'compensate')]


SCENECUT_DEFAULT = (64, 128, 4, 0, 1)  # the header's documented default
SCENECUT_STATE = ('cut', 'key', 'reason', 'dist', 'keys_by_cut', 'keys_by_period', 'keys_other', 'frames')


def scenecut_ok(params):
    """0 when every field of params (a Scenecut or five integers) is in its range, else -1 (None included);
    h264mi_scenecut_ok, host only"""
    return lib().h264mi_scenecut_ok(_byref(Scenecut._of(params)))


def scenecut_is_cut(params, stats):
    """1 when a frame's eight statistics words are a cut under params, 0 when not, -1 on bad parameters;
    h264mi_scenecut_is_cut, host only"""
    d = Scenecut._of(params)
    words = (ctypes.c_uint32 * 8)(*(int(v) for v in stats))
    return lib().h264mi_scenecut_is_cut(_byref(d), words)


def thumb_size(w, h):
    """(tw, th) = (ceil(w / 4), ceil(h / 4)) of a w x h frame (h264mi_thumb_size); ValueError on a bad side"""
    tw, th = ctypes.c_int(0), ctypes.c_int(0)
    if lib().h264mi_thumb_size(w, h, ctypes.byref(tw), ctypes.byref(th)) != 0:
        raise ValueError(f'bad size {w}x{h}')
    return tw.value, th.value


def i420_scenecut(cur, w, h, n, params, thumb_out=None, thumb_prev=None, stats=None, stream=None):
    """the thumbnails of n tight w x h I420 frames (uint8 CUDA tensor cur, any alignment) into thumb_out (n * tw * th
    bytes, may be thumb_prev itself or None) and, against the n thumbnails thumb_prev, their statistics into stats (a
    CUDA tensor of 8 n 32-bit words: {changed blocks, blocks, sum sad, sum Tc, sum Tp, 0, 0, 0}, zeroed and then
    accumulated on the stream); one launch, async on stream (default: the current one); h264mi_i420_scenecut_dev.
    params: a Scenecut or (level, share, min_gap, max_gap, compensate). The words and bytes equal tests/scenecutref.py's.
    ValueError on a bad argument."""
    _assert_dev_u8(cur)
    ok = n > 0 and min(w, h) > 0
    assert cur.numel() >= (n * _i420_bytes(w, h) if ok else 0)
    tb = n * ((w + 3) // 4) * ((h + 3) // 4) if ok else 0
    for t in (thumb_out, thumb_prev):
        if t is not None:
            _assert_dev_u8(t)
            assert t.numel() >= tb
    if stats is not None:
        assert stats.is_cuda and stats.is_contiguous() and stats.numel() * stats.element_size() >= 32 * max(n, 0)
    d = Scenecut._of(params)
    if lib().h264mi_i420_scenecut_dev(_ptr(stats), _ptr(thumb_out), _ptr(cur), _ptr(thumb_prev), w, h, n, _byref(d),
                                      _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {n} frames {w}x{h}, {d!r}')


class Deinterlace(_Record):
    """h264mi_deinterlace (include/h264mi.h): parity 0 (the even lines are kept) or 1, spatial 0 (linear) or 1
    (edge-directed), temporal 0 or 1 (weave where the previous frame shows no motion), comb_level 0..255 (the
    statistics' threshold). 16 bytes"""
    _fields_ = [(k, ctypes.c_int32) for k in ('parity', 'spatial', 'temporal', 'comb_level')]


def deinterlace_ok(params):
    """0 when every field of params (a Deinterlace or four integers) is in its range, else -1 (None included);
    h264mi_deinterlace_ok, host only"""
    return lib().h264mi_deinterlace_ok(_byref(Deinterlace._of(params)))


def i420_deinterlace(dst, cur, w, h, n, params, prev=None, prev_out=None, stats=None, stream=None):
    """n tight w x h I420 frames (uint8 CUDA tensor cur, any alignment) deinterlaced into dst; one launch, async on stream
    (default: the current one); h264mi_i420_deinterlace_dev. params: a Deinterlace or (parity, spatial, temporal,
    comb_level). prev, when given: the n previous unfiltered frames (without it the result is spatial only); prev_out,
    when given, receives the unfiltered cur; stats, when given: a CUDA tensor of 4 n 32-bit words, per frame {missing
    luma samples, combed luma samples, sum |O - v| over luma, over both chroma planes}, zeroed and then accumulated on
    the stream. dst may be exactly cur, prev_out exactly prev. The bytes equal tests/deintref.py's. ValueError on a bad
    argument (a parameter out of range, a side that is odd or outside 2..8192, n < 1, any other overlap of a written
    range)."""
    given = tuple(t for t in (dst, cur, prev, prev_out) if t is not None)
    _assert_dev_u8(*given)
    need = 0 if n <= 0 or min(w, h) <= 0 else n * _i420_bytes(w, h)
    assert all(t.numel() >= need for t in given)
    if stats is not None:
        assert stats.is_cuda and stats.is_contiguous() and stats.numel() * stats.element_size() >= 16 * max(n, 0)
    d = Deinterlace._of(params)
    if lib().h264mi_i420_deinterlace_dev(_ptr(dst), _ptr(prev_out), _ptr(cur), _ptr(prev), w, h, n, _byref(d),
                                         _ptr(stats), _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {n} frames {w}x{h}, {d!r}')


class Spatial(_Record):
    """h264mi_spatial (include/h264mi.h): radius_y, radius_c 0..3 (the binomial low-pass' radius; 0 copies), amount_y,
    amount_c -64..255 in 1/64 units (positive sharpens, negative blurs, -64 is the low-pass itself, 0 copies), core
    0..255 (with a positive amount, differences of at most core are left alone). 20 bytes"""
    _fields_ = [(k, ctypes.c_int32) for k in ('radius_y', 'radius_c', 'amount_y', 'amount_c', 'core')]


def spatial_ok(params):
    """0 when every field of params (a Spatial or five integers) is in its range, else -1 (None included);
    h264mi_spatial_ok, host only"""
    return lib().h264mi_spatial_ok(_byref(Spatial._of(params)))


def i420_spatial(dst, src, w, h, n, params, stream=None):
    """n tight w x h I420 frames (uint8 CUDA tensor src, any alignment) sharpened or blurred into dst; one launch, async
    on stream (default: the current one); h264mi_i420_spatial_dev. params: a Spatial or (radius_y, radius_c, amount_y,
    amount_c, core). Out of place only. The bytes equal tests/spatialref.py's. ValueError on a bad argument (a
    parameter out of range, a side that is odd or outside 2..8192, n < 1, buffers that share a byte)."""
    _assert_dev_u8(dst, src)
    need = 0 if n <= 0 or min(w, h) <= 0 else n * _i420_bytes(w, h)
    assert dst.numel() >= need and src.numel() >= need
    d = Spatial._of(params)
    if lib().h264mi_i420_spatial_dev(_ptr(dst), _ptr(src), w, h, n, _byref(d), _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {n} frames {w}x{h}, {d!r}')


LEVELS_AUTO = 0   # H264MI_LEVELS_AUTO: the ends are measured from each frame's luma histogram and smoothed
LEVELS_FIXED = 1  # H264MI_LEVELS_FIXED: the ends are in_lo and in_hi
LEVELS_RECORD = ('lo_m', 'hi_m', 'lo_s', 'hi_s', 'lo_e', 'hi_e', 'below', 'above')  # a frame's eight record words


class Levels(_Record):
    """h264mi_levels (include/h264mi.h): mode LEVELS_AUTO or LEVELS_FIXED, clip_lo, clip_hi 0..4096 (AUTO: the share of
    the luma samples, in 1/65536, that may fall below / above the measured end), in_lo < in_hi 0..255 (FIXED), out_lo <
    out_hi 0..255 (the range the ends are mapped to), max_gain 64..1024 (AUTO, in 1/64 units), speed 1..256 (AUTO; 256 =
    no memory), sat 0..255 (chroma gain about 128 in 1/64 units; 64 leaves chroma as it is). 40 bytes"""
    _fields_ = [(k, ctypes.c_int32) for k in ('mode', 'clip_lo', 'clip_hi', 'in_lo', 'in_hi', 'out_lo', 'out_hi', 'max_gain', 'speed', 'sat')]


def levels_ok(params):
    """0 when every field of params (a Levels or ten integers) is in its range, else -1 (None included);
    h264mi_levels_ok, host only"""
    return lib().h264mi_levels_ok(_byref(Levels._of(params)))


def levels_work_bytes(n):
    """the bytes of i420_levels' work tensor for n frames (h264mi_levels_work_bytes): n histograms, then n table sets"""
    return int(lib().h264mi_levels_work_bytes(int(n)))


def _assert_dev_words(t, nbytes):
    """t is None or a contiguous device tensor of at least nbytes bytes"""
    if t is not None:
        assert t.is_cuda and t.is_contiguous() and t.numel() * t.element_size() >= nbytes


def i420_hist(hist, frames, w, h, n, stream=None):
    """the histograms of n tight w x h I420 frames (uint8 CUDA tensor frames, any alignment) into hist (a CUDA tensor of
    768 n 32-bit words at a multiple of 4: per frame 256 counts of Y, of Cb, of Cr), zeroed and then accumulated on the
    stream; one launch, async on stream (default: the current one); h264mi_i420_hist_dev. The words equal
    tests/levelsref.py's. ValueError on a bad argument."""
    _assert_dev_u8(frames)
    ok = n > 0 and min(w, h) > 0
    assert frames.numel() >= (n * _i420_bytes(w, h) if ok else 0)
    _assert_dev_words(hist, 3072 * max(n, 0))
    if lib().h264mi_i420_hist_dev(_ptr(hist), _ptr(frames), w, h, n, _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {n} frames {w}x{h}')


def i420_lut(dst, src, w, h, n, luts, per_frame=False, stream=None):
    """n tight w x h I420 frames (uint8 CUDA tensor src, any alignment) through table sets of 768 bytes (T[0] for Y, T[1]
    for Cb, T[2] for Cr: O = T[plane][C]) into dst, which may be src itself; luts: one set for all frames, or with
    per_frame n sets; one launch, async on stream (default: the current one); h264mi_i420_lut_dev. The bytes equal
    tests/levelsref.py's. ValueError on a bad argument (dst and src that overlap in part, tables inside dst)."""
    _assert_dev_u8(dst, src, luts)
    need = 0 if n <= 0 or min(w, h) <= 0 else n * _i420_bytes(w, h)
    assert dst.numel() >= need and src.numel() >= need and luts.numel() >= 768 * (max(n, 1) if per_frame else 1)
    if lib().h264mi_i420_lut_dev(_ptr(dst), _ptr(src), w, h, n, _ptr(luts), 1 if per_frame else 0, _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {n} frames {w}x{h}, per_frame={per_frame}')


def i420_levels(dst, src, w, h, n, params, work, state=None, record=None, stream=None):
    """the levels of n tight w x h I420 frames that are n independent streams (uint8 CUDA tensor src, any alignment) into
    dst, which may be src itself; async on stream (default: the current one); h264mi_i420_levels_dev. params: a Levels
    or its ten integers. work: a CUDA tensor of levels_work_bytes(n) bytes at a multiple of 4. state: None (every frame
    is a first frame) or 4 n int32 words, read and advanced in AUTO mode; record: None or 8 n int32 words (LEVELS_RECORD).
    AUTO is the histogram, the decision and the tables' application; FIXED the last two. Bytes and words equal
    tests/levelsref.py's. ValueError on a bad argument."""
    _assert_dev_u8(dst, src)
    need = 0 if n <= 0 or min(w, h) <= 0 else n * _i420_bytes(w, h)
    assert dst.numel() >= need and src.numel() >= need
    _assert_dev_words(work, levels_work_bytes(n))
    _assert_dev_words(state, 16 * max(n, 0))
    _assert_dev_words(record, 32 * max(n, 0))
    d = Levels._of(params)
    if lib().h264mi_i420_levels_dev(_ptr(dst), _ptr(src), w, h, n, _byref(d), _ptr(state), _ptr(record), _ptr(work),
                                    _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {n} frames {w}x{h}, {d!r}')


PRIVACY_PIXELATE = 0  # H264MI_PRIVACY_PIXELATE: cells of block x block become their mean
PRIVACY_FILL = 1      # H264MI_PRIVACY_FILL: the rectangle becomes (fill_y, fill_cb, fill_cr)


WARP_CLAMP = 0  # H264MI_WARP_CLAMP: positions outside the source repeat its edge samples
WARP_FILL = 1   # H264MI_WARP_FILL: they take the fill values


class Warp(_Record):
    """h264mi_warp (include/h264mi.h): filter FILTER_BILINEAR or FILTER_BICUBIC, edge WARP_CLAMP or WARP_FILL, fill_y,
    fill_u, fill_v 0..255 (FILL), grid_log2 3..5 (the mesh pitch is 1 << grid_log2 destination luma samples). 24 bytes"""
    _fields_ = [(k, ctypes.c_int32) for k in ('filter', 'edge', 'fill_y', 'fill_u', 'fill_v', 'grid_log2')]


def warp_ok(params):
    """0 when every field of params (a Warp or six integers) is in its range, else -1 (None included); h264mi_warp_ok"""
    return lib().h264mi_warp_ok(_byref(Warp._of(params)))


def warp_mesh_size(dw, dh, grid_log2):
    """(mw, mh): the control points of a mesh for a dw x dh destination (h264mi_warp_mesh_size; host only). ValueError on a
    side that is odd or outside 2..8192 or grid_log2 outside 3..5."""
    mw, mh = ctypes.c_int(), ctypes.c_int()
    if lib().h264mi_warp_mesh_size(int(dw), int(dh), int(grid_log2), ctypes.byref(mw), ctypes.byref(mh)) != 0:
        raise ValueError(f'bad arguments: a mesh of pitch 1 << {grid_log2} for {dw}x{dh}')
    return mw.value, mh.value


def _warp_mesh(dw, dh, grid_log2, fill):
    """a (mh, mw, 2) int32 array filled by fill(pointer); ValueError when the builder refuses"""
    import numpy as np
    mw, mh = warp_mesh_size(dw, dh, grid_log2)
    mesh = np.zeros((mh, mw, 2), np.int32)
    if fill(mesh.ctypes.data_as(ctypes.c_void_p)) != mw * mh:
        raise ValueError(f'the builder refused its arguments for {dw}x{dh}, pitch 1 << {grid_log2}')
    return mesh


def warp_mesh_affine(dw, dh, grid_log2, m):
    """the mesh of the affine map m (six Q16 integers: x = m0 X + m1 Y + m2, y = m3 X + m4 Y + m5, in samples) as a
    (mh, mw, 2) numpy int32 array of (x, y) in sixteenths; h264mi_warp_mesh_affine, host only"""
    c = (ctypes.c_int32 * 6)(*(int(v) for v in m))
    return _warp_mesh(dw, dh, grid_log2, lambda p: lib().h264mi_warp_mesh_affine(p, int(dw), int(dh), int(grid_log2), c))


def warp_mesh_homography(dw, dh, grid_log2, h):
    """the mesh of the homography h (nine Q16 integers, row-major); ValueError where the denominator is not positive at a
    control point; h264mi_warp_mesh_homography, host only"""
    c = (ctypes.c_int32 * 9)(*(int(v) for v in h))
    return _warp_mesh(dw, dh, grid_log2, lambda p: lib().h264mi_warp_mesh_homography(p, int(dw), int(dh), int(grid_log2), c))


def warp_mesh_radial(dw, dh, grid_log2, cx, cy, r2, k1, k2):
    """the mesh that removes a two-coefficient radial lens distortion: (cx, cy) the centre in sixteenths, r2 the
    reference radius squared in sixteenths squared, k1, k2 signed Q16; ValueError beyond the limits the header states;
    h264mi_warp_mesh_radial, host only"""
    return _warp_mesh(dw, dh, grid_log2, lambda p: lib().h264mi_warp_mesh_radial(p, int(dw), int(dh), int(grid_log2), int(cx), int(cy),
                                                                                  int(r2), int(k1), int(k2)))


def warp_tile_class(mesh, dw, dh, sw, sh, grid_log2, plane, tx, ty):
    """0 when the kernel stages the source footprint of tile (tx, ty) of plane 0..2 in LDS, 1 when it samples global
    memory; mesh: a host (mh, mw, 2) int32 array; h264mi_warp_tile_class, host only"""
    import numpy as np
    m = np.ascontiguousarray(mesh, np.int32)
    assert m.size == 2 * int(np.prod(warp_mesh_size(dw, dh, grid_log2)))
    r = lib().h264mi_warp_tile_class(m.ctypes.data_as(ctypes.c_void_p), int(dw), int(dh), int(sw), int(sh), int(grid_log2), int(plane),
                                     int(tx), int(ty))
    if r < 0:
        raise ValueError(f'bad arguments: tile ({tx}, {ty}) of plane {plane}, {sw}x{sh} -> {dw}x{dh}')
    return r


def _assert_dev_mesh(mesh, dw, dh, d, count):
    """mesh is a contiguous int32 device tensor that holds count meshes (when the geometry is good enough to tell)"""
    import torch
    assert mesh.is_cuda and mesh.dtype == torch.int32 and mesh.is_contiguous()
    if d is not None and 3 <= d.grid_log2 <= 5 and min(dw, dh) > 0:
        G = 1 << d.grid_log2
        assert mesh.numel() >= count * 2 * ((dw + G - 1) // G + 1) * ((dh + G - 1) // G + 1)


def i420_warp(dst, src, sw, sh, dw, dh, n, mesh, params, mesh_per_frame=False, stream=None):
    """n tight sw x sh I420 frames (uint8 CUDA tensor src, any alignment) warped to n tight dw x dh frames (dst) under the
    mesh (int32 CUDA tensor: one mesh, or n back to back with mesh_per_frame), async on stream (default: the current
    one); h264mi_i420_warp_dev. params: a Warp or (filter, edge, fill_y, fill_u, fill_v, grid_log2). The bytes equal
    tests/warpref.py's. Minification is not antialiased. ValueError on a bad argument (a parameter out of range, a side
    that is odd or outside 2..8192, n < 1, a destination that shares a byte with the source or the mesh)."""
    _assert_dev_u8(dst, src)
    ok = n > 0 and min(sw, sh, dw, dh) > 0
    assert dst.numel() >= (n * _i420_bytes(dw, dh) if ok else 0) and src.numel() >= (n * _i420_bytes(sw, sh) if ok else 0)
    d = Warp._of(params)
    if ok:
        _assert_dev_mesh(mesh, dw, dh, d, n if mesh_per_frame else 1)
    if lib().h264mi_i420_warp_dev(_ptr(dst), int(dw), int(dh), _ptr(src), int(sw), int(sh), int(n), _ptr(mesh), int(bool(mesh_per_frame)),
                                  _byref(d), _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {n} frames {sw}x{sh} -> {dw}x{dh}, {d!r}')


def i420_warp_host(src, sw, sh, dw, dh, mesh, params):
    """one frame (a numpy uint8 array) warped on the host by the library's own loops (h264mi_i420_warp_host): the dw x dh
    frame as a numpy array. mesh: a host (mh, mw, 2) int32 array"""
    import numpy as np
    s = np.ascontiguousarray(src, np.uint8).ravel()
    m = np.ascontiguousarray(mesh, np.int32)
    d = Warp._of(params)
    assert s.size >= _i420_bytes(sw, sh) and m.size == 2 * int(np.prod(warp_mesh_size(dw, dh, d.grid_log2)))
    out = np.zeros(_i420_bytes(dw, dh), np.uint8)
    if lib().h264mi_i420_warp_host(out.ctypes.data_as(ctypes.c_void_p), int(dw), int(dh), s.ctypes.data_as(ctypes.c_void_p), int(sw), int(sh),
                                   m.ctypes.data_as(ctypes.c_void_p), _byref(d)) != 0:
        raise ValueError(f'bad arguments: {sw}x{sh} -> {dw}x{dh}, {d!r}')
    return out


class Privacy(_Record):
    """h264mi_privacy (include/h264mi.h): the even rectangle (x, y, w, h) of frame `frame`, mode PRIVACY_PIXELATE with
    block 4, 8, 16, 32 or 64, or PRIVACY_FILL with fill_y, fill_cb, fill_cr 0..255. 40 bytes"""
    _fields_ = [(k, ctypes.c_int32) for k in ('frame', 'x', 'y', 'w', 'h', 'mode', 'block', 'fill_y', 'fill_cb', 'fill_cr')]


def _privacy_array(masks):
    masks = [Privacy._of(m) for m in masks]
    return (Privacy * len(masks))(*masks)


def privacy_ok(masks, w, h, nframes):
    """0 when masks (a sequence of Privacy or ten-integer tuples) is a good list for nframes frames of w x h, else -1
    (an empty one included); h264mi_privacy_ok, host only"""
    arr = _privacy_array(masks or ())
    return lib().h264mi_privacy_ok(arr if len(arr) else None, len(arr), int(w), int(h), int(nframes))


def i420_privacy(frames, w, h, nframes, masks, stream=None):
    """the masks applied in place to nframes tight w x h I420 frames (uint8 CUDA tensor frames, any alignment); one
    launch per 64 masks, async on stream (default: the current one); h264mi_i420_privacy_dev. Samples outside the
    rectangles are never written. The bytes equal tests/spatialref.py's. ValueError on a list privacy_ok refuses."""
    _assert_dev_u8(frames)
    assert nframes <= 0 or min(w, h) <= 0 or frames.numel() >= nframes * _i420_bytes(w, h)
    arr = _privacy_array(masks or ())
    if lib().h264mi_i420_privacy_dev(_ptr(frames), int(w), int(h), int(nframes), arr if len(arr) else None, len(arr), _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {len(arr)} masks on {nframes} frames {w}x{h}')


PIX_I420 = 0  # H264MI_PIX_*: planes Y (w x h), Cb, Cr (w/2 x h/2)
PIX_NV12 = 1  # plane 0 Y; plane 1: h/2 rows of w bytes, byte 2i = Cb[i], 2i+1 = Cr[i]
PIX_NV21 = 2  # as NV12 with Cr first
PIX_YUY2 = 3  # one plane, h rows of 2w bytes: Y0 Cb Y1 Cr
PIX_UYVY = 4  # one plane: Cb Y0 Cr Y1
# 5..15 are unassigned and refused; the deeper and wider layouts (include/h264mi.h has their table):
PIX_I422, PIX_I444, PIX_NV16, PIX_Y800 = 16, 17, 18, 19  # 8 bit: planar 4:2:2 and 4:4:4, semi-planar 4:2:2, grey
PIX_P010, PIX_I010, PIX_P210, PIX_I210 = 20, 21, 22, 23  # 10 bit in 16-bit words: P* in bits 15..6, I* in bits 9..0
PIX_V210 = 24  # packed 10-bit 4:2:2, six pixels in four 32-bit words
DEPTH_ROUND, DEPTH_DITHER, DEPTH_TRUNC = 0, 1, 2  # H264MI_DEPTH_*: how 10 bits become 8
FMT_LAYOUT = 2  # H264MI_FMT_LAYOUT: what h264mi_dec_output_format reports while a layout is in effect


class PixLayout(ctypes.Structure):
    """h264mi_pix_layout (include/h264mi.h): row y of plane p of frame f starts at
    base + f * frame_stride + offset[p] + y * pitch[p]; entries of unused planes are 0. 48 bytes"""
    _fields_ = [('pix', ctypes.c_int32), ('pitch', ctypes.c_int32 * 3), ('offset', ctypes.c_int64 * 3), ('frame_stride', ctypes.c_int64)]

    def __init__(self, pix=0, pitch=(), offset=(), frame_stride=0):
        super().__init__()
        self.pix, self.frame_stride = pix, frame_stride
        for k, v in enumerate(pitch):
            self.pitch[k] = v
        for k, v in enumerate(offset):
            self.offset[k] = v

    def __repr__(self):
        return f'PixLayout(pix={self.pix}, pitch={list(self.pitch)}, offset={list(self.offset)}, frame_stride={self.frame_stride})'


class PixOpt(_Record):
    """h264mi_pixopt (include/h264mi.h): the depth rule (DEPTH_*) that 10-bit samples become 8-bit ones under; the
    reserved fields must be 0. 16 bytes"""
    _fields_ = [('depth', ctypes.c_int32), ('reserved', ctypes.c_int32 * 3)]

    def __init__(self, depth=0, reserved=(0, 0, 0)):
        super().__init__()
        self.depth = depth
        for k, v in enumerate(reserved):
            self.reserved[k] = v

    def __repr__(self):
        return f'PixOpt(depth={self.depth}, reserved={list(self.reserved)})'


def pixopt_ok(opt):
    """0 when depth is 0..2 and the reserved fields are 0, else -1 (None included); h264mi_pixopt_ok, host only"""
    return lib().h264mi_pixopt_ok(_byref(opt))


def pix_unit(pix):
    """the unit of format pix, 1, 2 or 4 bytes: what pitches, offsets, frame_stride and the base address are multiples
    of; -1 for an unknown format (h264mi_pix_unit; host only)"""
    return lib().h264mi_pix_unit(int(pix))


def pix_layout_tight(pix, w, h):
    """the tight layout of a w x h frame in format pix (PIX_*): pitch = row bytes, planes back to back, frame_stride =
    the span (h264mi_pix_layout_tight; host only). ValueError on an unknown format or a side that is odd or outside 2..8192."""
    out = PixLayout()
    if lib().h264mi_pix_layout_tight(ctypes.byref(out), int(pix), int(w), int(h)) != 0:
        raise ValueError(f'bad arguments: format {pix} of {w}x{h}')
    return out


def pix_span(layout, w, h):
    """bytes from a frame's base to one past the last byte the layout names, -1 on a bad layout (h264mi_pix_span; host only)"""
    return lib().h264mi_pix_span(ctypes.byref(layout), int(w), int(h))


def pix_layout_ok(layout, w, h):
    """0 when the layout can hold w x h frames, else -1 (h264mi_pix_layout_ok; host only)"""
    return lib().h264mi_pix_layout_ok(ctypes.byref(layout), int(w), int(h))


def _pix_fits(t, layout, w, h, n):
    """tensor t holds n frames of a good layout (a bad one is left to the library to refuse)"""
    return n <= 0 or pix_layout_ok(layout, w, h) != 0 or t.numel() >= (n - 1) * layout.frame_stride + pix_span(layout, w, h)


def pix_to_i420(dst, src, layout, w, h, n, stream=None, opt=None):
    """n w x h frames in `layout` (a PixLayout; uint8 CUDA tensor src, frame f at f * layout.frame_stride, any
    alignment that is a multiple of pix_unit) to n tight I420 frames (dst), one launch, async on stream (default: the
    current one); h264mi_pix_to_i420_opt_dev. I420, NV12 and NV21 samples are moved; 4:2:2 chroma is
    (rows 2y + 2y+1 + 1) >> 1, 4:4:4 chroma the rounded mean of each 2x2; 10-bit samples become 8-bit ones under opt (a
    PixOpt; None: DEPTH_ROUND): the bytes equal tests/pixref.py's and tests/pixdeepref.py's. ValueError on a bad
    argument (a layout pix_layout_ok refuses, an opt pixopt_ok refuses, n <= 0, overlapping buffers)."""
    _assert_dev_u8(dst, src)
    assert n <= 0 or min(w, h) <= 0 or (dst.numel() >= n * _i420_bytes(w, h) and _pix_fits(src, layout, w, h, n))
    if lib().h264mi_pix_to_i420_opt_dev(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()), ctypes.byref(layout), _byref(opt),
                                        w, h, n, _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {layout!r}, {opt!r}, {n} frames {w}x{h}')


def i420_to_pix(dst, layout, src, w, h, n, stream=None):
    """n tight w x h I420 frames (uint8 CUDA tensor src) to n frames in `layout` (dst, any alignment), one launch, async
    on stream; h264mi_i420_to_pix_dev. 4:2:2 chroma rows 2y and 2y+1 both take chroma row y. Bytes the layout does not
    name (pitch padding, gaps between planes and frames) are not written. ValueError as pix_to_i420."""
    _assert_dev_u8(dst, src)
    assert n <= 0 or min(w, h) <= 0 or (src.numel() >= n * _i420_bytes(w, h) and _pix_fits(dst, layout, w, h, n))
    if lib().h264mi_i420_to_pix_dev(ctypes.c_void_p(dst.data_ptr()), ctypes.byref(layout), ctypes.c_void_p(src.data_ptr()), w, h, n,
                                    _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {layout!r}, {n} frames {w}x{h}')


class Overlay(_Record):
    """h264mi_overlay (include/h264mi.h): the w x h crop at (sx, sy) of sprite `sprite` blended 1:1 onto canvas
    `canvas` at (dx, dy), its alpha scaled by opacity / 256; reserved is 0; 40 bytes"""
    _fields_ = [(k, ctypes.c_int32) for k in ('sprite', 'canvas', 'sx', 'sy', 'w', 'h', 'dx', 'dy', 'opacity', 'reserved')]


def _overlay_array(overlays):
    overlays = list(overlays)
    return (Overlay * len(overlays))(*overlays)


def i420a_bytes(w, h):
    """bytes of a tight w x h I420A sprite: Y, Cb, Cr, then a full-resolution alpha plane"""
    return 2 * w * h + 2 * (w // 2) * (h // 2)


def rgba_to_i420a(dst, src, w, h, n, stream=None, spec=None):
    """n tight RGBA8 frames (uint8 CUDA tensor src, 4-byte aligned) to n I420A sprites (dst, any alignment), one launch,
    async on stream (default: the current one); h264mi_rgba_to_i420a_dev. Y, Cb, Cr as rgba_to_i420, A the fourth byte.
    With spec (a ColorSpec) h264mi_rgba_to_i420a_cs_dev: Y, Cb, Cr as rgba_to_i420(..., spec=spec), which also refuses
    overlapping buffers. ValueError on a bad argument (an odd side or one outside 2..8192, n <= 0, a misaligned source)."""
    if spec is not None:
        return _convert_cs_dev(lib().h264mi_rgba_to_i420a_cs_dev, dst, src, i420a_bytes(w, h), w * h * 4, w, h, n, spec, stream)
    _assert_dev_u8(dst, src)
    assert n <= 0 or min(w, h) <= 0 or (dst.numel() >= n * i420a_bytes(w, h) and src.numel() >= n * w * h * 4)
    if lib().h264mi_rgba_to_i420a_dev(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()), w, h, n, _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {w}x{h}, {n} frames')


def i420_overlay(canvas, cw, ch, ncanvas, sprites, ow, oh, nsprites, overlays, stream=None):
    """every placement's crop of one of nsprites I420A sprites of ow x oh (uint8 CUDA tensor sprites) alpha-blended onto
    its rectangle of one of ncanvas tight cw x ch I420 frames (canvas), any alignment, async on stream (default: the
    current one); h264mi_i420_overlay_dev. Placements may overlap: list order, the last on top. Canvas bytes outside the
    rectangles keep their value. Exact integers: the bytes equal tests/overlayref.py's. ValueError on a bad argument
    (odd fields, a crop outside the sprite, a rectangle outside the canvas, opacity outside 0..256, reserved != 0,
    overlapping buffers, no placement or more than 4096)."""
    _assert_dev_u8(canvas, sprites)
    assert min(ncanvas, nsprites, ow, oh, cw, ch) <= 0 or (canvas.numel() >= ncanvas * _i420_bytes(cw, ch) and
                                                           sprites.numel() >= nsprites * i420a_bytes(ow, oh))
    arr = _overlay_array(overlays)
    if lib().h264mi_i420_overlay_dev(ctypes.c_void_p(canvas.data_ptr()), cw, ch, ncanvas, ctypes.c_void_p(sprites.data_ptr()), ow, oh,
                                     nsprites, arr, len(arr), _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {len(arr)} placements of {nsprites} sprites {ow}x{oh} on {ncanvas} canvases {cw}x{ch}')


def i420_fill(frames, w, h, n, y, cb, cr, stream=None):
    """n tight w x h I420 frames (uint8 CUDA tensor, any alignment) set to the colour (y, cb, cr), async on stream
    (default: the current one); h264mi_i420_fill_dev. ValueError on a bad argument."""
    _assert_dev_u8(frames)
    assert n <= 0 or min(w, h) <= 0 or frames.numel() >= n * _i420_bytes(w, h)
    if lib().h264mi_i420_fill_dev(ctypes.c_void_p(frames.data_ptr()), w, h, n, int(y), int(cb), int(cr), _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {n} frames {w}x{h}, colour ({y}, {cb}, {cr})')


def i420_quality(out, a, b, w, h, n, stream=None):
    """distortion records of n pairs of tight I420 frames (uint8 CUDA tensors a, b, any alignment) into out (a CUDA
    tensor of at least 64 * n bytes, 8-byte aligned: n h264mi_quality records), one launch, async on stream
    (default: the current one); h264mi_i420_quality_dev. Read them with quality_records()."""
    assert out.is_cuda and out.is_contiguous()
    _assert_dev_u8(a, b)
    fb = _i420_bytes(w, h)
    assert n <= 0 or (out.numel() * out.element_size() >= 64 * n and a.numel() >= n * fb and b.numel() >= n * fb)
    if lib().h264mi_i420_quality_dev(ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()),
                                     w, h, n, _hip_stream(stream)) != 0:
        raise ValueError(f'bad arguments: {w}x{h}, {n} pairs')


def quality_records(out, n):
    """the first n records of a tensor written by i420_quality, copied to the host as Quality structures
    (synchronises through the copy)"""
    raw = out.view(-1).cpu().numpy().tobytes()
    return [Quality.from_buffer_copy(raw[64 * k:64 * k + 64]) for k in range(n)]


def version():
    return lib().h264mi_version().decode()
