"""EuRoC MAV dataset reader + deterministic replay.

Counterpart of the reference's `streaming/dataset.py:12-219` (CSV/PNG readers, namedtuple messages,
start-time offset) and of `streaming/publisher.py:8-53` -- except that the wall-clock-paced publisher
threads are replaced by the deterministic sequential replay of SURVEY section 3.5 (IMU messages with
timestamp <= t are delivered before the stereo frame at t), which is what a throughput run needs and
what makes results reproducible.  PNGs are decoded with Pillow (the reference uses cv2.imread(path, -1),
dataset.py:110; OpenCV is not a dependency here).
"""
import os
from collections import namedtuple

import numpy as np

imu_msg = namedtuple('imu_msg', ['timestamp', 'angular_velocity', 'linear_acceleration'])
img_msg = namedtuple('img_msg', ['timestamp', 'image'])
stereo_msg = namedtuple('stereo_msg', ['timestamp', 'cam0_image', 'cam1_image', 'cam0_msg', 'cam1_msg'])
gt_msg = namedtuple('gt_msg', ['timestamp', 'p', 'q', 'v', 'bw', 'ba'])


def read_image(path):
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.ndim == 3:
        a = a[..., 0]
    if a.dtype != np.uint8:                      # cv2.imread(path, -1) of the reference would hand a uint16 array on: never truncate it silently
        raise ValueError('%s: %s image, expected uint8 (8-bit greyscale camera frames)' % (path, a.dtype))
    return np.ascontiguousarray(a)


class EuRoCDataset(object):
    """`EuRoCDataset(path)` with `.imu`, `.stereo`, `.groundtruth` iterables and
    `.set_starttime(offset)` (reference: dataset.py:189-219)."""

    def __init__(self, path):
        self.path = path
        m = os.path.join(path, 'mav0')
        self._imu_csv = os.path.join(m, 'imu0', 'data.csv')
        self._gt_csv = os.path.join(m, 'state_groundtruth_estimate0', 'data.csv')
        self._cam = [self._list_images(os.path.join(m, 'cam%d' % c, 'data')) for c in (0, 1)]
        self.timestamps = self._cam[0][1]
        self._imu = self._load_csv(self._imu_csv, 7)
        self._gt = self._load_csv(self._gt_csv, 17) if os.path.exists(self._gt_csv) else np.zeros((0, 17))
        # dataset.py:203: starttime = max(first imu, first stereo)
        self.starttime0 = max(self._imu[0, 0] if len(self._imu) else -np.inf, self.timestamps[0] if self.timestamps else -np.inf)
        self.starttime = self.starttime0

    @staticmethod
    def _list_images(d):
        names = sorted((n for n in os.listdir(d) if n.endswith('.png')), key=lambda n: float(n[:-4]))
        return [os.path.join(d, n) for n in names], [float(n[:-4]) * 1e-9 for n in names]

    @staticmethod
    def _load_csv(path, ncol):
        rows = []
        with open(path) as f:
            next(f)
            for line in f:
                v = [float(x) for x in line.strip().split(',')]
                if len(v) >= ncol:
                    rows.append(v[:ncol])
        a = np.array(rows, dtype=np.float64).reshape(-1, ncol)
        if len(a):
            a[:, 0] *= 1e-9                              # ns -> s (dataset.py:29,67)
        return a

    def set_starttime(self, offset):
        """dataset.py:206-214: everything before starttime0 + offset is skipped."""
        self.starttime = self.starttime0 + float(offset)

    @property
    def imu(self):
        for r in self._imu:
            if r[0] >= self.starttime:
                yield imu_msg(r[0], r[1:4].copy(), r[4:7].copy())

    @property
    def groundtruth(self):
        for r in self._gt:
            if r[0] >= self.starttime:
                yield gt_msg(r[0], r[1:4].copy(), r[4:8].copy(), r[8:11].copy(), r[11:14].copy(), r[14:17].copy())

    @property
    def stereo(self):
        (p0, t0), (p1, _t1) = self._cam
        for k in range(min(len(p0), len(p1))):
            if t0[k] < self.starttime:
                continue
            i0, i1 = read_image(p0[k]), read_image(p1[k])
            yield stereo_msg(t0[k], i0, i1, img_msg(t0[k], i0), img_msg(t0[k], i1))

    @property
    def stereo_files(self):
        """(timestamp, cam0 path, cam1 path) of every frame from the start time on -- what `stereo` decodes; the batch
        stager (`FrameStager`) decodes these on host threads one step ahead instead."""
        (p0, t0), (p1, _t1) = self._cam
        for k in range(min(len(p0), len(p1))):
            if t0[k] >= self.starttime:
                yield t0[k], p0[k], p1[k]

    def groundtruth_array(self):
        """float64[n, 8]: t, p(3), q as stored by EuRoC (w, x, y, z)."""
        g = self._gt[self._gt[:, 0] >= self.starttime]
        return g[:, :8].copy()


def _refuse_packed(who, fmt):
    """The packed 10 / 12-bit transports are what a camera link delivers, not what a file holds: no PNG flavour carries one, so nothing
    that reads or writes the EuRoC layout takes them (feed such frames to the engine directly: FrontendEngine, frontend.pack_frames)."""
    from . import _native as N
    if N.is_packed(fmt):
        raise ValueError('%s: %s is a packed transport, which no PNG file holds: the EuRoC reader, writer and stagers do not take it '
                         '(hand packed frames to FrontendEngine.step / step_host / frames_upload)' % (who, N.PIXEL_FORMAT_NAMES[fmt]))


def frame_array(pixel_format, n, height, width, zeros=True):
    """A host batch of n frames of a pixel format ('gray8' / 'gray16' / 'rgb8' / 'rgba8' / 'bayer_*8' / 'bayer_*16' or the AV_PIX_* code)
    as decode_batch fills it and the front-end takes it: uint8 [n, h, w], uint16 [n, h, w], uint8 [n, h, w, 3 | 4]; a Bayer mosaic is
    one sample per pixel, uint8 [n, h, w] or uint16 [n, h, w]."""
    from . import _native as N
    fmt = N.pixel_format_code(pixel_format)
    _refuse_packed('frame_array', fmt)
    bpp = N.PIXEL_BYTES[fmt]
    shape = (n, height, width) if bpp <= 2 else (n, height, width, bpp)
    return (np.zeros if zeros else np.empty)(shape, np.uint16 if N.is_16bit(fmt) else np.uint8)


def png_pixel_format(pixel_format):
    """The name of a pixel format that a PNG file can hold ('gray8', 'gray16', 'rgb8', 'rgba8'), from a name or an AV_PIX_* code.  PNG
    stores no BGR order: 'bgr8' / 'bgra8' are a ValueError here, so that RGB files are never handed to an engine that reads BGR.
    A raw Bayer mosaic on disk is a grey PNG: 'bayer_*8' gives 'gray8', 'bayer_*16' gives 'gray16' (the file cannot say that it is a
    mosaic; the engine's config.image_format does)."""
    from . import _native as N
    fmt = N.pixel_format_code(pixel_format)
    _refuse_packed('png_pixel_format', fmt)
    if N.is_bayer(fmt):
        return 'gray16' if N.is_16bit(fmt) else 'gray8'
    name = N.PIXEL_FORMAT_NAMES[fmt]
    if name not in ('gray8', 'gray16', 'rgb8', 'rgba8'):
        raise ValueError('PNG files hold gray8, gray16, rgb8 or rgba8 frames, not %s: decode such a sequence as rgb8 / rgba8 '
                         '(config.image_format) -- the files are in RGB order' % name)
    return name


def probe_png(path):
    """(width, height, format name or None) of a PNG file from its header alone (av_png_probe): 'gray8', 'gray16', 'rgb8', 'rgba8';
    None for a flavour the library's decoder does not take."""
    import ctypes as C
    from . import _native as N
    w, h, f = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    N.check(N.lib().av_png_probe(os.fsencode(path), C.byref(w), C.byref(h), C.byref(f)))
    return int(w.value), int(h.value), N.PIXEL_FORMAT_NAMES.get(int(f.value))


def _decode_batch_format(paths, out, threads):
    """decode_batch for the other flavours: out uint16 [n, h, w] (16-bit grey PNGs) or uint8 [n, h, w, 3 | 4] (RGB / RGBA PNGs), decoded
    by av_png_decode.  A file of any other flavour than the array's is an error naming it: nothing is converted on the host."""
    import ctypes as C
    from . import _native as N
    if out.ndim == 3 and out.dtype == np.uint16:
        fmt = N.AV_PIX_GRAY16
    elif out.ndim == 4 and out.dtype == np.uint8 and out.shape[3] in (3, 4):
        fmt = N.AV_PIX_RGB8 if out.shape[3] == 3 else N.AV_PIX_RGBA8
    else:
        raise ValueError('decode_batch: out must be uint8 [n, h, w], uint16 [n, h, w] or uint8 [n, h, w, 3 | 4], got %s %s' % (out.dtype, tuple(out.shape)))
    if not out.flags['C_CONTIGUOUS']:
        raise ValueError('decode_batch: out must be C-contiguous')
    idx = [i for i, p in enumerate(paths) if p is not None]
    if not idx:
        return
    h, w = out.shape[1:3]
    arr = (C.c_char_p * len(idx))(*[os.fsencode(paths[i]) for i in idx])
    status = (C.c_int32 * len(idx))()
    dst = out if len(idx) == out.shape[0] else np.empty((len(idx),) + out.shape[1:], out.dtype)
    rc = N.lib().av_png_decode(arr, len(idx), w, h, fmt, dst.ctypes.data_as(C.c_void_p), dst[0].nbytes, int(threads), status)
    if rc == N.AV_E_CAPACITY:
        bad = [paths[i] for k, i in enumerate(idx) if status[k] == 1]
        raise ValueError('%s: not a %d x %d %s PNG (the batch is decoded as %s)' % (bad[0], w, h, N.PIXEL_FORMAT_NAMES[fmt], N.PIXEL_FORMAT_NAMES[fmt]))
    N.check(rc)
    if dst is not out:
        out[idx] = dst


def decode_batch(paths, out, threads=16):
    """Decode len(paths) greyscale PNG files into out[i] (uint8 [n, h, w], C-contiguous) on `threads` host threads with the
    library's decoder (av_png_decode_gray8: zlib + PNG row filters in C++, no GIL); a file of another PNG flavour (16-bit,
    RGB, palette ...) is decoded by Pillow.  paths[i] = None leaves out[i] untouched.
    out uint16 [n, h, w] decodes 16-bit grey PNGs, out uint8 [n, h, w, 3 | 4] RGB / RGBA PNGs (av_png_decode); there a file of another
    flavour than the array's is a ValueError."""
    import ctypes as C
    from . import _native as N
    if not (out.ndim == 3 and out.dtype == np.uint8):
        return _decode_batch_format(paths, out, threads)
    idx = [i for i, p in enumerate(paths) if p is not None]
    if not idx:
        return
    n, h, w = out.shape
    assert out.flags['C_CONTIGUOUS'] and out.dtype == np.uint8
    arr = (C.c_char_p * len(idx))(*[os.fsencode(paths[i]) for i in idx])
    status = (C.c_int32 * len(idx))()
    if len(idx) == n:
        dst, tmp = out, None
    else:
        tmp = np.empty((len(idx), h, w), np.uint8); dst = tmp
    rc = N.lib().av_png_decode_gray8(arr, len(idx), w, h, dst.ctypes.data_as(C.c_void_p), h * w, int(threads), status)
    if rc == N.AV_E_CAPACITY:                 # some file is not 8-bit greyscale: that file alone goes through Pillow
        for k, i in enumerate(idx):
            if status[k] == 1:
                im = np.asarray(read_image(paths[i]))
                if im.dtype != np.uint8 or im.shape != (h, w):         # e.g. a 16-bit PNG: never truncated silently
                    raise ValueError('%s: %s %s image, expected uint8 %s' % (paths[i], im.dtype, im.shape, (h, w)))
                dst[k] = im
            elif status[k] != 0:
                N.check(N.AV_E_INVALID)
    else:
        N.check(rc)
    if tmp is not None:
        out[idx] = tmp


class FrameStager(object):
    """Batch staging for sweeps (reference: the reader threads of streaming/dataset.py:93-158): the frames of
    step k+1 of all S streams are decoded on host threads while step k runs on the GPU.  `next()` returns
    (timestamps float64[S] (-1 = stream finished), img0 uint8[S,h,w], img1) of the next step, or None when every stream
    is done; the arrays stay valid until the call after the next one (three buffers: one being filled by the
    loader thread, the one just returned, the one returned before it)."""

    def __init__(self, datasets, height, width, max_frames=None, threads=16, pixel_format='gray8'):
        """pixel_format: the flavour of the files and of the arrays returned (frame_array): 'gray8', 'gray16', 'rgb8', 'rgba8'; a Bayer
        name reads the grey flavour that holds the mosaic (png_pixel_format)."""
        from concurrent.futures import ThreadPoolExecutor
        self.S = len(datasets)
        self.its = [iter(d.stereo_files) for d in datasets]
        one = frame_array(png_pixel_format(pixel_format), self.S, height, width)
        self.buf = [np.zeros((2,) + one.shape, one.dtype) for _ in range(3)]      # [slot][camera][stream]
        self.max_frames, self.threads, self.k = max_frames, threads, 0
        self._files, self.last_files = {}, None          # last_files: [(cam0 path, cam1 path) or None per stream] of the step `next` last returned
        self.pool = ThreadPoolExecutor(1)
        self.fut = self.pool.submit(self._load, 0)

    def _load(self, k):
        if self.max_frames is not None and k >= self.max_frames:
            return None
        ent = [next(it, None) for it in self.its]
        if all(e is None for e in ent):
            return None
        ts = np.array([-1.0 if e is None else e[0] for e in ent])
        self._files[k] = [None if e is None else (e[1], e[2]) for e in ent]
        buf = self.buf[k % 3]
        both = [None if e is None else e[1] for e in ent] + [None if e is None else e[2] for e in ent]
        decode_batch(both, buf.reshape((2 * self.S,) + buf.shape[2:]), self.threads)     # cam0 and cam1 of all streams in one threaded call
        for s, e in enumerate(ent):
            if e is None:
                buf[:, s] = 0                    # a finished stream idles on blank images
        return ts, buf[0], buf[1]

    def next(self):
        res = self.fut.result()
        self.last_files = self._files.pop(self.k, None)
        self.k += 1
        self.fut = self.pool.submit(self._load, self.k) if res is not None else None
        return res

    def close(self):
        if self.fut is not None:
            try:
                self.fut.result()
            except Exception:
                pass
        self.pool.shutdown(wait=True)


class SharedFramePlan(object):
    """Which DISTINCT frames a batch of streams reads at which step, and where each lives in the front-end's device frame store
    (`FrontendEngine.frames_*`).  The reference's sweep replays one sequence from several start offsets (run.bat:4-12; an offset
    only moves the start index, dataset.py:206-214): stream i reads frame start_i + k at step k, so every frame is read by every
    offset stream a few steps apart -- here it is decoded, uploaded, pyramided and FAST-scanned once, when the first of them
    reaches it, and dropped when the last has tracked away from it.  Streams of different sequences simply share nothing.

    Frames are keyed by their (cam0 path, cam1 path).  Computed up front from the datasets' file lists:
      n_steps, n_slots            steps of the longest stream; store entries needed (the most frames ever live at once)
      slots[k]    int32[S]        store entry stream s reads at step k; -1 = the stream is over
      ts[k]       float64[S]      frame time; -1 = over
      new[k]      [(entry, cam0 path, cam1 path)]   frames first read at step k: upload them before the step (at the earliest
                                  right before step k - 1 is enqueued: an entry is handed out again only two steps after its last reader)
    A frame is read as the current image at step k and as the previous image at step k + 1 of the same stream."""

    def __init__(self, datasets, max_frames=None):
        files = []
        for d in datasets:
            f = list(d.stereo_files)
            files.append(f if max_frames is None else f[:max_frames])
        S = self.S = len(files)
        self.n_steps = max([len(f) for f in files] + [0])
        last_need = {}
        for f in files:
            for k, (_t, p0, p1) in enumerate(f):
                need = k + 1 if k + 1 < len(f) else k
                key = (p0, p1)
                if last_need.get(key, -1) < need:
                    last_need[key] = need
        self.slots = np.full((self.n_steps, S), -1, np.int32)
        self.ts = np.full((self.n_steps, S), -1.0)
        self.new = [[] for _ in range(self.n_steps)]
        import heapq
        free, where, n_slots = [], {}, 0             # free: heap of (first step the entry may be rewritten for, entry)
        for k in range(self.n_steps):
            for s, f in enumerate(files):
                if k >= len(f):
                    continue
                t, p0, p1 = f[k]
                key = (p0, p1)
                e = where.get(key)
                if e is None:
                    if free and free[0][0] <= k:
                        e = heapq.heappop(free)[1]
                    else:
                        e = n_slots; n_slots += 1
                    where[key] = e
                    self.new[k].append((e, p0, p1))
                self.slots[k, s] = e
                self.ts[k, s] = t
            for key in [key for key, e in where.items() if last_need[key] == k]:
                heapq.heappush(free, (k + 2, where.pop(key)))
        self.n_slots = max(n_slots, 1)
        self.n_frames_distinct = sum(len(n) for n in self.new)
        self.n_stream_frames = int((self.slots >= 0).sum())


class SharedFrameStager(object):
    """Decodes the NEW frames of every step of a `SharedFramePlan` on host threads, a few steps ahead of the GPU (reference: the
    reader threads of streaming/dataset.py:93-158).  `get(k)` -> (entries int32[n], img0 uint8[n,h,w], img1) of step k; steps must be
    asked for in order."""

    def __init__(self, plan, height, width, threads=16, ahead=3, pixel_format='gray8'):
        """pixel_format: the flavour of the files and of the arrays returned (frame_array): 'gray8', 'gray16', 'rgb8', 'rgba8'; a Bayer
        name reads the grey flavour that holds the mosaic (png_pixel_format)."""
        from concurrent.futures import ThreadPoolExecutor
        self.plan, self.h, self.w, self.threads, self.ahead = plan, height, width, threads, ahead
        self.pixel_format = png_pixel_format(pixel_format)
        self.pool = ThreadPoolExecutor(1)
        self.futs = {}
        self.submitted = 0
        self._fill(0)

    def _decode(self, k):
        new = self.plan.new[k]
        n = len(new)
        buf = frame_array(self.pixel_format, 2 * n, self.h, self.w, zeros=False)
        if n:
            decode_batch([e[1] for e in new] + [e[2] for e in new], buf, self.threads)
        return np.array([e[0] for e in new], np.int32), buf[:n], buf[n:]

    def _fill(self, k):
        while self.submitted < min(self.plan.n_steps, k + 1 + self.ahead):
            self.futs[self.submitted] = self.pool.submit(self._decode, self.submitted)
            self.submitted += 1

    def get(self, k):
        self._fill(k)
        res = self.futs.pop(k).result()
        self._fill(k + 1)
        return res

    def close(self):
        for f in self.futs.values():
            try:
                f.result()
            except Exception:
                pass
        self.pool.shutdown(wait=True)


class ExposureTimes(object):
    """The exposure time of every frame of sequences in the EuRoC layout that hold `mav0/cam0/times.txt` and `mav0/cam1/times.txt` next
    to each camera's `data` directory.  The layout is that of the `times.txt` of the TUM mono-VO dataset -- one line per frame,
        <file stem> <timestamp in s> <exposure in ms>
    separated by white space; empty lines and lines that start with `#` are skipped -- and this text is the contract: the files of
    that dataset were not at hand to check it against.  A line is matched to its PNG by the first column, which is the file's name
    without `.png` (compared as text).  `of(png path)` returns the exposure of that frame in ms; the file of a camera is read once, when
    the first of its frames is asked for.  ValueError naming the times.txt: a file that is missing, a line that does not hold three
    columns with a finite exposure > 0, a stem listed twice, a frame without a line."""

    def __init__(self):
        self._cams = {}

    @staticmethod
    def times_path(png_path):
        return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(png_path))), 'times.txt')

    @staticmethod
    def read(path):
        if not os.path.isfile(path):
            raise ValueError('exposure times: %s is missing (one line per frame: <file stem> <timestamp in s> <exposure in ms>)' % path)
        out = {}
        with open(path) as f:
            for no, line in enumerate(f, 1):
                col = line.split()
                if not col or col[0].startswith('#'):
                    continue
                try:
                    if len(col) != 3:
                        raise ValueError
                    float(col[1])
                    e = float(col[2])
                    if not (np.isfinite(e) and e > 0):
                        raise ValueError
                except ValueError:
                    raise ValueError('exposure times: %s line %d is not <file stem> <timestamp in s> <exposure in ms> with an exposure > 0: %r' % (path, no, line.strip()))
                if col[0] in out:
                    raise ValueError('exposure times: %s lists frame %s twice' % (path, col[0]))
                out[col[0]] = e
        return out

    def of(self, png_path):
        path = self.times_path(png_path)
        if path not in self._cams:
            self._cams[path] = self.read(path)
        stem = os.path.basename(png_path)
        stem = stem[:-4] if stem.endswith('.png') else stem
        if stem not in self._cams[path]:
            raise ValueError('exposure times: %s has no line for frame %s' % (path, stem))
        return self._cams[path][stem]

    def check(self, datasets, max_frames=None):
        """Every frame the datasets will hand out has its line, in both cameras' files: found before the first step."""
        for d in datasets:
            for k, (_t, p0, p1) in enumerate(d.stereo_files):
                if max_frames is not None and k >= max_frames:
                    break
                self.of(p0), self.of(p1)
        return self


def replay(dataset, imu_sinks, on_stereo, max_frames=None):
    """Deterministic replay: for each stereo frame at time t deliver every IMU message with
    timestamp <= t to each sink (order of vio.py:43-44), then call on_stereo(msg)."""
    it = iter(dataset.imu)
    pending = next(it, None)
    n = 0
    for msg in dataset.stereo:
        while pending is not None and pending.timestamp <= msg.timestamp:
            for sink in imu_sinks:
                sink(pending)
            pending = next(it, None)
        on_stereo(msg)
        n += 1
        if max_frames is not None and n >= max_frames:
            break
    return n


BAYER_GAINS = (0.8, 1.0, 0.6)                    # default R, G, B gains of a synthetic mosaic (encode_frame)


def bayer_site_colours(pixel_format, height, width):
    """int [h, w]: the colour (0 R, 1 G, 2 B) of every site of a Bayer format, from the colours of its top-left 2 x 2 block."""
    from . import _native as N
    fmt = N.pixel_format_code(pixel_format)
    if not N.is_bayer(fmt):
        raise ValueError('%r is no Bayer mosaic format' % (pixel_format,))
    block = np.array(['RGB'.index(ch) for ch in N.BAYER_PATTERNS[(fmt - 16) & 3].upper()]).reshape(2, 2)      # [y & 1, x & 1]
    yy, xx = np.mgrid[0:height, 0:width]
    return block[yy & 1, xx & 1]


def encode_frame(image, pixel_format='gray8', gains=BAYER_GAINS, shift=8):
    """An 8-bit grey frame as a frame of another format.  'gray16' = g << 8, 'rgb8' / 'rgba8' / 'bgr8' / 'bgra8' = equal colour channels
    (alpha 255): these convert back to the frame exactly.  A Bayer format gives the raw mosaic of a scene whose R, G, B are the grey
    value times `gains`: every site holds rint(g * gain of its colour) clipped to 255, as uint8 [..., h, w], or that value << shift as
    uint16 for the 16-bit mosaics (config.gray16_shift = shift reads it back)."""
    from . import _native as N
    fmt = N.pixel_format_code(pixel_format)
    _refuse_packed('encode_frame', fmt)
    g = np.asarray(image, np.uint8)
    if fmt == N.AV_PIX_GRAY8:
        return g
    if N.is_bayer(fmt):
        gain = np.asarray(gains, np.float64)[bayer_site_colours(fmt, g.shape[-2], g.shape[-1])]
        m = np.clip(np.rint(g.astype(np.float64) * gain), 0, 255).astype(np.uint8)
        return m.astype(np.uint16) << N.gray16_shift_value(shift) if N.is_16bit(fmt) else m
    if fmt == N.AV_PIX_GRAY16:
        return g.astype(np.uint16) << 8
    out = np.repeat(g[..., None], N.PIXEL_BYTES[fmt], axis=-1)
    if N.PIXEL_BYTES[fmt] == 4:
        out[..., 3] = 255
    return out


def write_euroc_layout(root, stream, groundtruth_rate_hz=200.0, frame_range=None, write_csv=True, compress_level=6, pixel_format='gray8',
                       bayer_gains=BAYER_GAINS, gray16_shift=8, vignette=None, exposure=None):
    """Write a seeded synthetic stream (uav_airvision_amd.synth.SyntheticStream) as an EuRoC-layout directory
    `root/mav0/{cam0,cam1}/data/<ns>.png`, `imu0/data.csv`, `state_groundtruth_estimate0/data.csv`, so that the same
    reader / replay / sweep code that runs on the real dataset (which is not redistributable and not present on the build
    or GPU boxes) can be exercised end to end.  PNG is lossless: the reader returns the rendered pixels bit for bit.
    Ground truth = the analytic trajectory of the stream (position of the IMU frame; identity orientation columns).
    `frame_range=(a, b)` writes only the images of frames a..b-1 (several writer processes can share one sequence);
    `write_csv=False` skips the IMU / ground-truth files; `compress_level` is zlib's (any level is lossless; 1 writes 5x faster).
    `pixel_format` 'gray16' / 'rgb8' / 'rgba8' writes the same frames as 16-bit grey / RGB / RGBA PNGs (encode_frame); a Bayer name
    writes the raw mosaic of the frames coloured by `bayer_gains` as 8- or 16-bit grey PNGs (16-bit samples << `gray16_shift`).
    `vignette` = (V0, V1) or (V0, V1, response_forward): every frame of cam0 / cam1 is degraded with frontend.apply_vignette before it is
    encoded (what a vignetting lens and a non-linear sensor would have recorded); None writes the frames as they are.
    `exposure` = (t0, t1, t_ref): frame k of cam0 / cam1 is recorded at an exposure of t0[k] / t1[k] ms by a camera whose frames as
    rendered are at t_ref -- frontend.apply_exposure with the ratio t / t_ref, behind the vignette and the response of `vignette` if
    given -- and `mav0/cam0/times.txt` and `mav0/cam1/times.txt` list the frames this call wrote (`ExposureTimes` has the layout)."""
    from PIL import Image
    from . import _native as N
    if pixel_format in N.PACKED_FORMATS:
        _refuse_packed('write_euroc_layout', N.PACKED_FORMATS[pixel_format])
    bayer = pixel_format in N.PIXEL_FORMATS and N.is_bayer(N.PIXEL_FORMATS[pixel_format])
    if pixel_format not in ('gray8', 'gray16', 'rgb8', 'rgba8') and not bayer:
        raise ValueError('write_euroc_layout: PNG holds gray8, gray16, rgb8 or rgba8 frames or a Bayer mosaic, not %r' % (pixel_format,))
    enc = (lambda im: encode_frame(im, pixel_format, bayer_gains, gray16_shift)) if bayer else (lambda im: encode_frame(im, pixel_format))
    deg0 = deg1 = (lambda im: im)
    if vignette is not None:
        from .frontend import apply_vignette
        forward = vignette[2] if len(vignette) > 2 else None
        deg0, deg1 = (lambda im: apply_vignette(im, vignette[0], forward)), (lambda im: apply_vignette(im, vignette[1], forward))
    for cam in ('cam0', 'cam1'):
        os.makedirs(os.path.join(root, 'mav0', cam, 'data'), exist_ok=True)
    a, b = (0, stream.n_frames) if frame_range is None else frame_range
    times = ([], [])
    for k in range(a, b):
        m = stream.frame(k)
        stem = '%d' % int(round(m.timestamp * 1e9))
        name = stem + '.png'
        im0, im1 = m.cam0_image, m.cam1_image
        if exposure is not None:
            from .frontend import apply_exposure
            t0, t1, t_ref = exposure
            v = (None, None, None) if vignette is None else (vignette[0], vignette[1], vignette[2] if len(vignette) > 2 else None)
            im0 = apply_exposure(im0, float(t0[k]) / float(t_ref), v[0], v[2])
            im1 = apply_exposure(im1, float(t1[k]) / float(t_ref), v[1], v[2])
            times[0].append('%s %.9f %r\n' % (stem, m.timestamp, float(t0[k])))
            times[1].append('%s %.9f %r\n' % (stem, m.timestamp, float(t1[k])))
        else:
            im0, im1 = deg0(im0), deg1(im1)
        Image.fromarray(enc(im0)).save(os.path.join(root, 'mav0', 'cam0', 'data', name), compress_level=compress_level)
        Image.fromarray(enc(im1)).save(os.path.join(root, 'mav0', 'cam1', 'data', name), compress_level=compress_level)
    if exposure is not None:
        for cam in (0, 1):
            with open(os.path.join(root, 'mav0', 'cam%d' % cam, 'times.txt'), 'w') as f:
                f.writelines(times[cam])
    if not write_csv:
        return root
    os.makedirs(os.path.join(root, 'mav0', 'imu0'), exist_ok=True)
    with open(os.path.join(root, 'mav0', 'imu0', 'data.csv'), 'w') as f:
        f.write('#timestamp [ns],w_RS_S_x [rad s^-1],w_RS_S_y [rad s^-1],w_RS_S_z [rad s^-1],a_RS_S_x [m s^-2],a_RS_S_y [m s^-2],a_RS_S_z [m s^-2]\n')
        for m in stream.imu:
            f.write('%d,%.12f,%.12f,%.12f,%.12f,%.12f,%.12f\n' % (int(round(m.timestamp * 1e9)), *m.angular_velocity, *m.linear_acceleration))
    os.makedirs(os.path.join(root, 'mav0', 'state_groundtruth_estimate0'), exist_ok=True)
    with open(os.path.join(root, 'mav0', 'state_groundtruth_estimate0', 'data.csv'), 'w') as f:
        f.write('#timestamp,p_RS_R_x [m],p_RS_R_y [m],p_RS_R_z [m],q_RS_w [],q_RS_x [],q_RS_y [],q_RS_z [],v_RS_R_x,v_RS_R_y,v_RS_R_z,bw_x,bw_y,bw_z,ba_x,ba_y,ba_z\n')
        t_begin, t_end = stream.imu[0].timestamp, stream.imu[-1].timestamp
        n = int((t_end - t_begin) * groundtruth_rate_hz) + 1
        for i in range(n):
            t = t_begin + i / groundtruth_rate_hz
            p = stream.position(t)
            f.write(','.join(['%d' % int(round(t * 1e9))] + ['%.9f' % v for v in p] + ['1', '0', '0', '0'] + ['0'] * 9) + '\n')
    return root
