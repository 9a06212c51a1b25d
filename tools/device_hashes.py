#!/usr/bin/env python3
"""md5 of the .text and .rodata sections of every device code object of libh264mi (CPU only, no GPU needed): each
translation unit compiled device-only with the library's flags, the two sections extracted as raw bytes. Two trees
whose tables are equal run the same device code. Usage: device_hashes.py [tree root] > table.txt"""
import hashlib
import os
import subprocess
import sys
import tempfile

UNITS = ('h264mi_kernels', 'quality', 'scale', 'compose', 'overlay', 'upscale', 'orient', 'pixfmt', 'pixdeep', 'colorspace', 'denoise', 'scenecut', 'deinterlace', 'spatial', 'levels', 'warp')
HIPCC = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only', '--no-gpu-bundle-output', '-c']
OBJCOPY = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin', 'llvm-objcopy')


def section_md5(obj, section, tmp):
    raw = os.path.join(tmp, 'section.bin')
    subprocess.run([OBJCOPY, '-O', 'binary', '--only-section=' + section, obj, raw], check=True)
    with open(raw, 'rb') as f:
        data = f.read()
    return hashlib.md5(data).hexdigest(), len(data)


def main():
    root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, 'openh264-wasm_amd', 'csrc')
    print(f'{"unit":<16}{"section":<9}{"bytes":>9}  md5')
    with tempfile.TemporaryDirectory() as tmp:
        for u in UNITS:
            if not os.path.exists(os.path.join(csrc, u + '.hip')):  # a tree from before the unit existed
                print(f'{u:<16}absent')
                continue
            obj = os.path.join(tmp, u + '.dev')
            subprocess.run(HIPCC + ['-Wno-unused-result', '-Wno-pass-failed', os.path.join(csrc, u + '.hip'), '-o', obj], check=True)
            for sec in ('.text', '.rodata'):
                md5, n = section_md5(obj, sec, tmp)
                print(f'{u:<16}{sec:<9}{n:>9}  {md5}')


if __name__ == '__main__':
    main()
