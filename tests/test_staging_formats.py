"""Host-side staging of the other PNG flavours (av_png_decode, av_png_probe): 16-bit grey, RGB and RGBA files against Pillow on every
row filter type at bytes-per-pixel 2, 3 and 4, and the frame stager on a 16-bit EuRoC-layout sequence.  Host code only: no GPU needed."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from uav_airvision_amd import _native as N
from uav_airvision_amd.euroc import EuRoCDataset, FrameStager, decode_batch, frame_array, probe_png, write_euroc_layout

FLAVOURS = {'gray8': (8, 0, 1), 'gray16': (16, 0, 2), 'rgb8': (8, 2, 3), 'rgba8': (8, 6, 4)}      # bit depth, colour type, bytes per pixel


def _file_bytes(img, fmt):
    """The sample bytes of an image as the PNG holds them, [h, w * bpp]: 16-bit samples big-endian."""
    h, w = img.shape[:2]
    if fmt == 'gray16':
        return img.astype('>u2').view(np.uint8).reshape(h, 2 * w)
    return np.ascontiguousarray(img).reshape(h, -1)


def write_png(path, img, fmt, filters, level=6, idat=1 << 30):
    """A PNG of flavour `fmt` whose row r uses filter type filters[r] (spec 9.2, any bytes per pixel): a and c are bpp bytes back."""
    depth, colour, bpp = FLAVOURS[fmt]
    h, w = img.shape[:2]
    a = _file_bytes(img, fmt).astype(np.int32)
    n = a.shape[1]
    left = np.concatenate([np.zeros((h, bpp), np.int32), a[:, :n - bpp]], 1) if n > bpp else np.zeros_like(a)
    up = np.concatenate([np.zeros((1, n), np.int32), a[:-1]], 0)
    ul = np.concatenate([np.zeros((h, bpp), np.int32), up[:, :n - bpp]], 1) if n > bpp else np.zeros_like(a)
    pp = left + up - ul
    pa, pb, pc = np.abs(pp - left), np.abs(pp - up), np.abs(pp - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    pred = [np.zeros_like(a), left, up, (left + up) >> 1, paeth]
    rows = b''.join(bytes([f]) + ((a[r] - pred[f][r]) & 0xFF).astype(np.uint8).tobytes() for r, f in enumerate(filters))
    z = zlib.compress(rows, level)

    def chunk(t, d):
        return struct.pack('>I', len(d)) + t + d + struct.pack('>I', zlib.crc32(t + d) & 0xFFFFFFFF)
    open(path, 'wb').write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, colour, 0, 0, 0))
                           + b''.join(chunk(b'IDAT', z[i:i + idat]) for i in range(0, len(z), idat)) + chunk(b'IEND', b''))


def make_image(rng, fmt, h, w):
    """Smooth structure plus noise, so that every filter type has something to predict; every bit of a 16-bit sample used."""
    base = 120 + 50 * np.sin(np.arange(w) / 9.0)[None, :] + 30 * np.cos(np.arange(h) / 5.0)[:, None]
    if fmt == 'gray16':
        return np.clip(base * 256 + rng.normal(0, 900, (h, w)), 0, 65535).astype(np.uint16)
    c = FLAVOURS[fmt][2]
    return np.clip(base[..., None] + rng.normal(0, 25, (h, w, c)) + np.arange(c) * 17, 0, 255).astype(np.uint8)


def pillow(path, fmt):
    with Image.open(path) as im:
        a = np.asarray(im)
    return a.astype(np.uint16) if fmt == 'gray16' else a


def decode(paths, fmt, h, w, threads=4):
    out = frame_array(fmt, len(paths), h, w)
    out[:] = 0xA5
    decode_batch(paths, out, threads=threads)
    return out


def cases(tmp_path, rng):
    """(path, fmt, h, w, image): every flavour x each filter type forced on all rows, mixed runs, widths 1, 7, 16, 33 and one 752 x 480."""
    out = []
    for fmt in ('gray16', 'rgb8', 'rgba8'):
        k = 0
        for (h, w) in ((11, 1), (9, 7), (12, 16), (10, 33)):
            for filt in (0, 1, 2, 3, 4, 'mixed'):
                img = make_image(rng, fmt, h, w)
                f = [int(v) for v in rng.integers(0, 5, h)] if filt == 'mixed' else [filt] * h
                p = str(tmp_path / ('%s_%d.png' % (fmt, k)))
                write_png(p, img, fmt, f, level=[1, 6, 9][k % 3], idat=(1 << 30) if k % 2 else 97)
                out.append((p, fmt, h, w, img))
                k += 1
        img = make_image(rng, fmt, 480, 752)
        f = []
        run = 1
        while len(f) < 480:                       # runs of each type of every length 1 .. 12, the first row Paeth
            f += [(4 + len(f)) % 5] * run
            run = run % 12 + 1
        p = str(tmp_path / ('%s_full.png' % fmt))
        write_png(p, img, fmt, f[:480], idat=5000)
        out.append((p, fmt, 480, 752, img))
    return out


def test_the_writer_is_a_valid_encoder_and_the_decoder_matches_pillow(tmp_path):
    rng = np.random.default_rng(21)
    for p, fmt, h, w, img in cases(tmp_path, rng):
        ref = pillow(p, fmt)
        assert ref.shape == img.shape and np.array_equal(ref, img), p          # Pillow reads what was written
        got = decode([p], fmt, h, w)[0]
        assert got.dtype == img.dtype and np.array_equal(got, img), p


def test_pillow_written_files_and_holes(tmp_path):
    rng = np.random.default_rng(22)
    for fmt in ('gray16', 'rgb8', 'rgba8'):
        imgs = [make_image(rng, fmt, 480, 752) for _ in range(3)]
        paths = []
        for i, a in enumerate(imgs):
            p = str(tmp_path / ('%s_p%d.png' % (fmt, i)))
            Image.fromarray(a).save(p, compress_level=[1, 6, 9][i], optimize=bool(i & 1))
            paths.append(p)
        out = decode(paths, fmt, 480, 752)
        for a, o in zip(imgs, out):
            assert np.array_equal(o, a)
        out2 = frame_array(fmt, 3, 480, 752)
        out2[:] = 7
        decode_batch([paths[0], None, paths[2]], out2, threads=2)
        assert np.array_equal(out2[0], imgs[0]) and (out2[1] == 7).all() and np.array_equal(out2[2], imgs[2])


@pytest.mark.parametrize('backend', ['libdeflate', 'zlib'])
def test_both_inflate_back_ends(tmp_path, backend):
    """AV_PNG_ZLIB is read when the library is first used: a child process decodes the same files with either back end."""
    import subprocess, sys, textwrap
    rng = np.random.default_rng(23)
    args = []
    for p, fmt, h, w, img in cases(tmp_path, rng):
        if h == 480 or w == 33:
            np.save(p[:-4] + '.npy', img)
            args.append('%s,%s,%d,%d' % (p, fmt, h, w))
    code = textwrap.dedent("""
        import sys, numpy as np
        from uav_airvision_amd.euroc import decode_batch, frame_array
        for a in sys.argv[1:]:
            path, fmt, h, w = a.split(','); h = int(h); w = int(w)
            out = frame_array(fmt, 1, h, w)
            decode_batch([path], out)
            assert np.array_equal(out[0], np.load(path[:-4] + '.npy')), path
        print('ok')
    """)
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    env.pop('AV_PNG_ZLIB', None)
    if backend == 'zlib':
        env['AV_PNG_ZLIB'] = '1'
    r = subprocess.run([sys.executable, '-c', code] + args, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'ok' in r.stdout, r.stderr[-2000:]


def _raw_decode(paths, fmt, h, w):
    arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
    status = (C.c_int32 * len(paths))()
    out = frame_array(fmt, len(paths), h, w)
    rc = N.lib().av_png_decode(arr, len(paths), w, h, N.pixel_format_code(fmt), out.ctypes.data_as(C.c_void_p), out[0].nbytes, 2, status)
    return rc, list(status), out


def test_status_codes(tmp_path):
    rng = np.random.default_rng(24)
    h, w = 40, 52
    files = {}
    for fmt in FLAVOURS:
        img = make_image(rng, fmt, h, w) if fmt != 'gray8' else rng.integers(0, 256, (h, w), dtype=np.uint8)
        files[fmt] = str(tmp_path / (fmt + '.png'))
        write_png(files[fmt], img, fmt, [int(v) for v in rng.integers(0, 5, h)])
    # every flavour decodes as itself and is status 1 (not the flavour asked for) as any other
    for want in FLAVOURS:
        rc, st, _ = _raw_decode([files[f] for f in FLAVOURS], want, h, w)
        assert rc == N.AV_E_CAPACITY and st == [0 if f == want else 1 for f in FLAVOURS], (want, st)
        assert _raw_decode([files[want]], want, h, w)[:2] == (0, [0])
    assert _raw_decode([files['rgb8']], 'rgb8', h, w + 1)[:2] == (N.AV_E_CAPACITY, [1])           # another size
    with pytest.raises(ValueError, match='gray16'):
        decode_batch([files['gray16'], files['rgb8']], frame_array('gray16', 2, h, w))
    # the old entry point keeps refusing a 16-bit file
    out8 = np.zeros((1, h, w), np.uint8)
    arr = (C.c_char_p * 1)(os.fsencode(files['gray16']))
    st1 = (C.c_int32 * 1)()
    assert N.lib().av_png_decode_gray8(arr, 1, w, h, out8.ctypes.data_as(C.c_void_p), h * w, 1, st1) == N.AV_E_CAPACITY and st1[0] == 1
    # truncated file, flipped bit inside the compressed data, missing file: status 2
    data = open(files['rgb8'], 'rb').read()
    cut = str(tmp_path / 'cut.png'); open(cut, 'wb').write(data[:len(data) // 2])
    flip = bytearray(data); flip[len(data) // 2] ^= 0x10
    bad = str(tmp_path / 'flip.png'); open(bad, 'wb').write(bytes(flip))
    rc, st, _ = _raw_decode([files['rgb8'], cut, bad, str(tmp_path / 'missing.png')], 'rgb8', h, w)
    assert rc == N.AV_E_INVALID and st == [0, 2, 2, 2]
    with pytest.raises(N.AirvisionError, match='corrupt|truncated'):
        decode_batch([files['rgb8'], cut], frame_array('rgb8', 2, h, w))
    # formats PNG has no flavour for, and a stride smaller than an image
    for fmt in (N.AV_PIX_BGR8, N.AV_PIX_BGRA8, 6, -1):
        arr = (C.c_char_p * 1)(os.fsencode(files['rgb8']))
        o = np.zeros((1, h, w, 4), np.uint8)
        assert N.lib().av_png_decode(arr, 1, w, h, fmt, o.ctypes.data_as(C.c_void_p), o.nbytes, 1, None) == N.AV_E_INVALID
    o = np.zeros((1, h, w, 3), np.uint8)
    assert N.lib().av_png_decode(arr, 1, w, h, N.AV_PIX_RGB8, o.ctypes.data_as(C.c_void_p), h * w * 3 - 1, 1, None) == N.AV_E_INVALID


def test_probe(tmp_path):
    rng = np.random.default_rng(25)
    for k, fmt in enumerate(FLAVOURS):
        h, w = 5 + k, 9 + 2 * k
        img = make_image(rng, fmt, h, w) if fmt != 'gray8' else rng.integers(0, 256, (h, w), dtype=np.uint8)
        p = str(tmp_path / (fmt + '.png'))
        Image.fromarray(img).save(p)
        assert probe_png(p) == (w, h, fmt)
    pal = str(tmp_path / 'pal.png')
    Image.fromarray(rng.integers(0, 256, (6, 6), dtype=np.uint8)).convert('P').save(pal)
    assert probe_png(pal) == (6, 6, None)                                            # a flavour the decoder does not take: no error, no format
    la = str(tmp_path / 'la.png')
    Image.fromarray(rng.integers(0, 256, (6, 7, 2), dtype=np.uint8), 'LA').save(la)
    assert probe_png(la) == (7, 6, None)
    junk = str(tmp_path / 'junk.png'); open(junk, 'wb').write(b'not a png at all, but long enough to hold a header')
    with pytest.raises(N.AirvisionError, match='not a PNG'):
        probe_png(junk)
    with pytest.raises(N.AirvisionError, match='cannot open'):
        probe_png(str(tmp_path / 'missing.png'))


def test_frame_stager_on_a_16_bit_sequence(tmp_path, cfg):
    from uav_airvision_amd.synth import SyntheticStream
    st = SyntheticStream(cfg, seed=4, n_frames=4)
    root = write_euroc_layout(str(tmp_path / 'S16'), st, pixel_format='gray16', compress_level=1)
    ds = EuRoCDataset(root)
    files = list(ds.stereo_files)
    assert len(files) == 4 and probe_png(files[0][1]) == (752, 480, 'gray16')
    stager = FrameStager([ds, EuRoCDataset(root)], 480, 752, threads=4, pixel_format='gray16')
    try:
        for k in range(4):
            ts, i0, i1 = stager.next()
            m = st.frame(k)
            assert i0.dtype == np.uint16 and i0.shape == (2, 480, 752)
            for s in range(2):
                assert np.array_equal(i0[s], m.cam0_image.astype(np.uint16) << 8) and np.array_equal(i1[s], m.cam1_image.astype(np.uint16) << 8)
        assert stager.next() is None
    finally:
        stager.close()
    with pytest.raises(ValueError, match='gray8, gray16, rgb8 or rgba8'):
        write_euroc_layout(str(tmp_path / 'X'), st, pixel_format='bgr8')
