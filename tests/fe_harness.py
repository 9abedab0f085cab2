"""tests/fe_harness.py -- TEST INFRASTRUCTURE ONLY: what every "front-end engine against the CPU oracle" test stands on, once: configs
with attributes set, replayable streams (rendered once, with other images, raw frames with their reference conversion), the oracle
loop, the engine loop over its five entry paths, and the frame-by-frame comparison of the two."""
import numpy as np

MODES = ('step', 'persist', 'prestage', 'host', 'frames')
TRACKED = ('before_tracking', 'after_tracking', 'after_matching')      # OracleFrontend.num_features, set by _track (frame 1 on)
ADDED = ('n_fast', 'n_candidates', 'n_new')                            # OracleFrontend.debug['add'], set by _add_new (frame 1 on)


def make_cfg(**kw):
    from uav_airvision_amd.config import ConfigEuRoC
    cfg = ConfigEuRoC()
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def scaled_cfg(w, h, **kw):
    """ConfigEuRoC for the same rig with w x h sensors, then the attributes."""
    from uav_airvision_amd.synth import scaled_config
    cfg = scaled_config(make_cfg(), w, h)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def bare_cfg(dropped):
    """A plain object with every attribute of ConfigEuRoC() but those whose name `dropped` says yes to: what a caller's config from
    before a switch existed looks like."""
    class Bare(object):
        pass
    bare = Bare()
    for k, v in vars(make_cfg()).items():
        if not dropped(k):
            setattr(bare, k, v)
    return bare


# ---- streams -------------------------------------------------------------------------------------------------------------------
def with_images(m, a, b):
    """The stereo message `m` with other images: same timestamp, same message types."""
    return type(m)(m.timestamp, a, b, type(m.cam0_msg)(m.timestamp, a), type(m.cam1_msg)(m.timestamp, b))


class Frames(object):
    """A stream held in memory: `.imu`, `.n_frames`, `.frame(k)` as synth.replay and the runners below read them; `.raw[k]` =
    (timestamp, raw cam0, raw cam1) where the stream has raw frames (`.frame(k)` is then their reference conversion)."""

    def __init__(self, base, frames, raw=None):
        self.imu, self.n_frames, self._frames = base.imu, len(frames), frames
        if raw is not None:
            self.raw = raw
        for name in ('in_moving_region', 'position'):          # what callers read of a SyntheticStream besides its frames
            if hasattr(base, name):
                setattr(self, name, getattr(base, name))

    def frame(self, k):
        return self._frames[k]

    @classmethod
    def cached(cls, stream, n_frames=None):
        """`stream` (anything with .imu, .n_frames, .frame(k)) with its first n frames rendered once."""
        return cls(stream, [stream.frame(k) for k in range(stream.n_frames if n_frames is None else n_frames)])

    def map(self, fn, n_frames=None):
        """The same stream with fn applied to both images of its first n frames."""
        return Frames(self, [with_images(m, fn(m.cam0_image), fn(m.cam1_image)) for m in self._frames[:n_frames]])

    @classmethod
    def raw_twin(cls, base, encode, convert, n_frames, post=None):
        """The first n frames of `base` as raw frames, encode(image), and their reference conversion post(convert(raw)): what the
        engine is fed (`.raw`) and what the unmodified oracle, or a gray8 engine, is fed (`.frame`)."""
        raw, conv = [], []
        for k in range(n_frames):
            m = base.frame(k)
            r0, r1 = encode(m.cam0_image), encode(m.cam1_image)
            a, b = convert(r0), convert(r1)
            if post is not None:
                a, b = post(a), post(b)
            raw.append((m.timestamp, r0, r1))
            conv.append(with_images(m, a, b))
        return cls(base, conv, raw)


# ---- the two loops -------------------------------------------------------------------------------------------------------------
def run_oracle(cfg, stream, n_frames=None, oracle=None, extra=None):
    """Replays `stream` through `oracle` (an OracleFrontend or a subclass of it; None: a plain one for cfg).  Per frame
    dict(ids, uv, nf, add) and whatever extra(oracle, feature message) adds; `add` is empty where the oracle did not run its adder."""
    from oracle.frontend import OracleFrontend
    from uav_airvision_amd.synth import replay
    fe = OracleFrontend(cfg) if oracle is None else oracle
    out = []

    def on_frame(m):
        msg = fe.stereo_callback(m)
        ids = np.array([f.id for f in msg.features], np.int64)
        uv = np.array([[f.u0, f.v0, f.u1, f.v1] for f in msg.features], np.float64).reshape(-1, 4)
        out.append(dict(ids=ids, uv=uv, nf=dict(fe.num_features), add=dict(fe.debug.get('add', {})), **(extra(fe, msg) if extra else {})))

    class Head(object):
        imu, frame = stream.imu, staticmethod(stream.frame)
    Head.n_frames = stream.n_frames if n_frames is None else n_frames
    replay(Head, [fe.imu_callback], on_frame)
    return out


def read_ransac_counts(eng, i):
    return (eng.read_ransac_counts(i),)


def read_grid(eng, i):
    return (eng.read_grid(i),)


def run_engine(cfg, streams, mode='step', n_frames=None, raw=False, max_corners=None, timing=False, images_of=None, read=None):
    """One FrontendEngine over `streams` through one entry path: every IMU sample up to a frame's time, then the frame.  raw feeds
    stream.raw[k] instead of stream.frame(k).  Returns per stream a list of (ids, uv, counters, *read(eng, stream index)) per frame;
    with images_of = a stream index also what read_image gave for both cameras of that stream on every frame; with timing the span
    counts per class of every step.  The caller's arrays and tensors are compared with copies after every step and upload."""
    import torch
    from uav_airvision_amd.frontend import FrontendEngine
    assert mode in MODES, mode
    S = len(streams)
    n_frames = streams[0].n_frames if n_frames is None else n_frames
    eng = FrontendEngine(cfg, n_streams=S, max_corners=max_corners, inputs_persist=mode in ('persist', 'prestage'))
    if mode == 'frames':
        eng.frames_reserve(2 * S + 1)
    if timing:
        eng.enable_timing(64)
    out, images, spans = [[] for _ in streams], [], []
    its = [iter(s.imu) for s in streams]
    pend = [next(it, None) for it in its]

    def arrays(k):
        if raw:
            ts, c0, c1 = zip(*[s.raw[k] for s in streams])
        else:
            ts, c0, c1 = zip(*[(m.timestamp, m.cam0_image, m.cam1_image) for m in [s.frame(k) for s in streams]])
        return np.stack(c0), np.stack(c1), list(ts)
    dev = {}
    for k in range(n_frames):
        a0, a1, ts = arrays(k)
        for i in range(S):
            while pend[i] is not None and pend[i].timestamp <= ts[i]:
                eng.push_imu(i, pend[i].timestamp, pend[i].angular_velocity)
                pend[i] = next(its[i], None)
        if mode in ('step', 'persist', 'prestage'):
            if k not in dev:
                dev[k] = (torch.from_numpy(a0).cuda(), torch.from_numpy(a1).cuda())
            eng.step(dev[k][0], dev[k][1], ts)
        else:
            h0, h1 = a0.copy(), a1.copy()
            if mode == 'host':
                eng.step_host(h0, h1, ts)
            else:
                # entries out of order and away from the upload's own positions, so that whatever is indexed has to follow the list
                slots = (np.arange(S, dtype=np.int32)[::-1] + 1 + (k & 1) * S).astype(np.int32)
                eng.frames_upload(slots, h0, h1)
            assert np.array_equal(h0, a0) and np.array_equal(h1, a1), (mode, k)
            if mode == 'frames':
                eng.step_frames(slots, ts)
        feats = eng.read_features()
        for i in range(S):
            out[i].append((feats[i][0], feats[i][1], eng.read_counters(i)) + (tuple(read(eng, i)) if read else ()))
        if images_of is not None:
            images.append((eng.read_image(images_of, 0), eng.read_image(images_of, 1)))
        if timing:
            spans.append({c: v[1] for c, v in eng.read_timing().items()})
        if k in dev:                                  # the caller's tensors are what they were
            assert np.array_equal(dev[k][0].cpu().numpy(), a0) and np.array_equal(dev[k][1].cpu().numpy(), a1), (mode, k)
            if mode == 'prestage' and k + 1 < n_frames:
                b0, b1, _ts = arrays(k + 1)
                dev[k + 1] = (torch.from_numpy(b0).cuda(), torch.from_numpy(b1).cuda())
                eng.prestage(*dev[k + 1])
            dev.pop(k - 1, None)
    eng.close()
    res = [out]
    if images_of is not None:
        res.append(images)
    if timing:
        res.append(spans)
    return res[0] if len(res) == 1 else tuple(res)


# ---- comparisons ---------------------------------------------------------------------------------------------------------------
def same(a, b):
    """Two frames of run_engine: ids, uv as bit patterns, and every further element equal."""
    return len(a) == len(b) and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) and \
        all(x == y for x, y in zip(a[2:], b[2:]))


def against_oracle(ref, got, tag, images=None, frames=None, min_features=None, floor_from=0):
    """One stream of run_engine against run_oracle's frames, on every frame: no overflow, ids equal, uv equal as bit patterns,
    n_published = their number; from frame 1 the tracker's counters against `nf` (a key the oracle did not set is 0); wherever the
    oracle ran its adder (`add` not empty: frame 1 on, and frame 0 of an oracle whose first-frame stage records it) the adder's
    counters.  images (run_engine's, with images_of) are those of frames.frame(k), shape and content, both cameras.  min_features:
    the fewest features a frame from floor_from on may publish, so that the comparison is not vacuous."""
    assert len(ref) == len(got) > 0, (tag, len(ref), len(got))
    for k, (r, g) in enumerate(zip(ref, got)):
        ids, uv, cnt = g[0], g[1], g[2]
        where = '%s frame %d' % (tag, k)
        assert cnt['overflow'] == 0, where
        assert np.array_equal(ids, r['ids']), where
        assert uv.shape == r['uv'].shape and np.array_equal(uv.view(np.uint64), r['uv'].view(np.uint64)), where
        assert cnt['n_published'] == len(r['ids']), (where, cnt)
        if k > 0:
            assert [cnt[c] for c in TRACKED] == [r['nf'].get(c, 0) for c in TRACKED], (where, cnt, r['nf'])
        if r['add']:
            assert [cnt[c] for c in ADDED] == [r['add'][c] for c in ADDED], (where, cnt, r['add'])
        if images is not None:
            m = frames.frame(k)
            for im, want in ((images[k][0], m.cam0_image), (images[k][1], m.cam1_image)):
                assert im.shape == want.shape and np.array_equal(im, want), where
        if min_features is not None and k >= floor_from:
            assert len(ids) >= min_features, (where, len(ids))
