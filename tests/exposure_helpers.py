"""tests/exposure_helpers.py -- TEST INFRASTRUCTURE ONLY: what the exposure tests add to tests/fe_harness.py.  Streams whose frames
carry exposure times (`.exposure[k]` = (t0, t1)), degraded by the forward model of tests/exposure_ref.py, with their reference-corrected
twins; and the engine loop of fe_harness.run_engine with the exposures handed to every entry path."""
import numpy as np

import exposure_ref as er
from fe_harness import MODES, Frames, with_images

T_REF = 8.0                   # the reference exposure of the tests, "ms"


def exposed_stream(base, n_frames, ratios, tables=None, vignette=None, forward=None, encode=None, convert=None, post=None):
    """The first n frames of `base` as an auto-exposing rig records them: camera c of frame k exposes for ratios[c][k] * T_REF behind its
    vignette[c] and sensor forward[c] (None: neither).  `.raw[k]` = (timestamp, cam0, cam1) as the engine is fed them (encode()d if
    given), `.exposure[k]` = (t0, t1), and `.frame(k)` the reference twin post(correct(convert(raw))) with camera c's integer tables
    tables[c] = (response, gain) (None: no tables) and the frame's own factor: what the unmodified oracle is fed."""
    raw, conv, expo = [], [], []
    for k in range(n_frames):
        m = base.frame(k)
        t = [ratios[c][k] * T_REF for c in (0, 1)]
        r = [er.degrade(im, ratios[c][k], None if vignette is None else vignette[c], None if forward is None else forward[c])
             for c, im in enumerate((m.cam0_image, m.cam1_image))]
        if encode is not None:
            r = [encode(x) for x in r]
        q = [(None, None) if tables is None else tables[c] for c in (0, 1)]
        g = [er.correct(x if convert is None else convert(x), q[c][0], q[c][1], int(er.quantise(t[c], T_REF))) for c, x in enumerate(r)]
        if post is not None:
            g = [post(x) for x in g]
        raw.append((m.timestamp, r[0], r[1]))
        conv.append(with_images(m, g[0], g[1]))
        expo.append((t[0], t[1]))
    st = Frames(base, conv, raw)
    st.exposure = expo
    return st


def run_engine(cfg, streams, mode='step', n_frames=None, max_corners=None, timing=False, images_of=None, exposures=True):
    """fe_harness.run_engine (raw frames) with exposure=(e0, e1) of the streams' frames handed to every call that hands frames over:
    `step`, `step_host`, `frames_upload`, and in 'prestage' mode the prestage (the step that follows it gets none).  exposures=False:
    no keyword at all (an engine without config.exposure_reference).  Returns what fe_harness.run_engine returns, and per stream and
    frame what read_exposure gave as the last element of its tuple when exposures are on."""
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
        ts, c0, c1 = zip(*[s.raw[k] for s in streams])
        return np.stack(c0), np.stack(c1), list(ts)

    def expo(k):
        if not exposures:
            return {}
        return dict(exposure=(np.array([s.exposure[k][0] for s in streams]), np.array([s.exposure[k][1] for s in streams])))
    dev, prestaged = {}, set()
    for k in range(n_frames):
        a0, a1, ts = arrays(k)
        for i in range(S):
            while pend[i] is not None and pend[i].timestamp <= ts[i]:
                eng.push_imu(i, pend[i].timestamp, pend[i].angular_velocity)
                pend[i] = next(its[i], None)
        if mode in ('step', 'persist', 'prestage'):
            if k not in dev:
                dev[k] = (torch.from_numpy(a0).cuda(), torch.from_numpy(a1).cuda())
            eng.step(dev[k][0], dev[k][1], ts, **({} if k in prestaged else expo(k)))
        else:
            h0, h1 = a0.copy(), a1.copy()
            if mode == 'host':
                eng.step_host(h0, h1, ts, **expo(k))
            else:
                slots = (np.arange(S, dtype=np.int32)[::-1] + 1 + (k & 1) * S).astype(np.int32)
                eng.frames_upload(slots, h0, h1, **expo(k))
            assert np.array_equal(h0, a0) and np.array_equal(h1, a1), (mode, k)
            if mode == 'frames':
                eng.step_frames(slots, ts)
        feats = eng.read_features()
        for i in range(S):
            out[i].append((feats[i][0], feats[i][1], eng.read_counters(i)) + ((eng.read_exposure(i),) if exposures else ()))
        if images_of is not None:
            images.append((eng.read_image(images_of, 0), eng.read_image(images_of, 1)))
        if timing:
            spans.append({c: v[1] for c, v in eng.read_timing().items()})
        if k in dev:                                  # the caller's tensors are what they were
            assert np.array_equal(dev[k][0].cpu().numpy(), a0) and np.array_equal(dev[k][1].cpu().numpy(), a1), (mode, k)
            if mode == 'prestage' and k + 1 < n_frames:
                b0, b1, _ts = arrays(k + 1)
                dev[k + 1] = (torch.from_numpy(b0).cuda(), torch.from_numpy(b1).cuda())
                eng.prestage(*dev[k + 1], **expo(k + 1))
                prestaged.add(k + 1)
            dev.pop(k - 1, None)
    eng.close()
    res = [out]
    if images_of is not None:
        res.append(images)
    if timing:
        res.append(spans)
    return res[0] if len(res) == 1 else tuple(res)
