"""CPU: the RGBA surface of the batch API exists at every layer -- declared in include/h264mi.h, exported by the
library, bound and mirrored in Python -- and the device conversions refuse bad arguments before touching a device."""
import ctypes

from test_capi_exports import declared_functions

NEW = ('h264mi_rgba_to_i420_dev', 'h264mi_i420_to_rgba_dev', 'h264mi_enc_encode_rgba', 'h264mi_enc_rgba_frame_bytes',
       'h264mi_dec_set_output_format', 'h264mi_dec_output_format')


def test_header_declares_and_library_exports(libpath):
    names = declared_functions()
    L = ctypes.CDLL(libpath)
    for n in NEW:
        assert n in names, n
        assert hasattr(L, n), n


def test_dev_conversions_refuse_bad_arguments_without_a_device(libpath):
    import h264mi
    L = h264mi.lib()
    a, b = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)  # never dereferenced: every call below is refused first
    for fn in (L.h264mi_rgba_to_i420_dev, L.h264mi_i420_to_rgba_dev):
        assert fn(a, b, 15, 16, 1, None) == -1
        assert fn(a, b, 16, 15, 1, None) == -1
        assert fn(a, b, 0, 16, 1, None) == -1
        assert fn(a, b, 16, -16, 1, None) == -1
        assert fn(a, b, 16, 16, 0, None) == -1
        assert fn(a, b, 16, 16, -3, None) == -1
        assert fn(None, b, 16, 16, 1, None) == -1
        assert fn(a, None, 16, 16, 1, None) == -1
    # null handles: refused, and the size query of no encoder is 0
    assert L.h264mi_enc_encode_rgba(None, a) == -1
    assert L.h264mi_enc_rgba_frame_bytes(None) == 0
    assert L.h264mi_dec_set_output_format(None, 1) == -1
    assert L.h264mi_dec_output_format(None) == -1


def test_python_mirror(libpath):
    import h264mi
    assert callable(h264mi.BatchEncoder.encode_rgba)
    assert callable(h264mi.BatchDecoder.set_output_format) and callable(h264mi.BatchDecoder.output_format)
    assert h264mi.BatchDecoder.OUTPUT_FORMATS == {'i420': 0, 'rgba': 1}
    assert callable(h264mi.rgba_to_i420) and callable(h264mi.i420_to_rgba)
    doc = h264mi.BatchDecoder.decode_frames.__doc__
    assert 'w * h * 4' in doc and 'w * h * 3 // 2' in doc
