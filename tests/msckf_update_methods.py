"""tests/msckf_update_methods.py -- TEST INFRASTRUCTURE ONLY.

Plain fp64 numpy.linalg / scipy.linalg statements of the three METHODS the batched update back end takes, as the comments of
csrc/msckf.hip and csrc/msckf_mfma.inc document them -- not transcriptions of the kernels: no tiles, no masks, no task maps, library
factorisations.  They are where the bars of the compressed and the information-form paths come from (msckf_update_cases): the oracle's
thin QR is a different and better-conditioned algorithm and cannot say what those two methods cost in fp64.

Every function takes Hc = H[:, cols] (m x nc), r (m), P (n x n), cols and the observation noise s^2 and returns (delta_x, P+).

stack_rule is the integer rule of upd_stack_kernel, and reference_loop the reference's own loop (msckf.py:658-668), for the tests that
hold the one to the other.
"""
import numpy as np
from scipy.linalg import solve_triangular

KCH = 136                   # DEV_KCH: stacked rows one back-end pass takes directly
INFO_NC, INFO_MAXROWS = 24, 8192
STACK_BLOCKS = 4096         # STACK_LDS_BLOCKS
BAD_PIVOT = -2              # UPD_BAD_PIVOT


def direct(Hc, r, P, cols, s2):
    """Cholesky of S = H P H^T + s^2 I, forward substitution of [P[:, c] Hc^T | r], P - Y^T Y (msckf_mfma.inc, the head comment)."""
    Hc, r, P = np.asarray(Hc, float), np.asarray(r, float), np.asarray(P, float)
    T = P[:, cols] @ Hc.T                                    # n x k
    S = Hc @ T[cols, :] + s2 * np.eye(len(Hc))
    L = np.linalg.cholesky((S + S.T) / 2)
    Y = solve_triangular(L, np.concatenate([T.T, r[:, None]], axis=1), lower=True)
    Yt = Y[:, :-1]
    Pn = P - Yt.T @ Yt
    return Yt.T @ Y[:, -1], (Pn + Pn.T) / 2


def regulariser(A):
    """E of the row compression: 1e-12 of the LARGEST diagonal entry of the Gram matrix, on every diagonal entry."""
    return 1e-12 * np.max(np.diag(A)) + 1e-300


def compress_rows(Hc, r):
    """(F, f) with F^T F = A + E, F^T f = b from the Cholesky factor of the bordered Gram matrix [A + E, b; b^T, 2 rho + 1] (msckf.hip,
    "Row compression WITHOUT a QR"; E and the border above chol_mfma_body)."""
    Hc, r = np.asarray(Hc, float), np.asarray(r, float)
    nc = Hc.shape[1]
    G = np.concatenate([Hc, r[:, None]], axis=1)
    B = G.T @ G
    B[:nc, :nc] += regulariser(B[:nc, :nc]) * np.eye(nc)
    B[nc, nc] = 2 * B[nc, nc] + 1
    L = np.linalg.cholesky(B)
    return L[:nc, :nc].T.copy(), L[nc, :nc].copy()


def compression(Hc, r, P, cols, s2):
    """Gram matrix, bordered Cholesky with E, then the direct method on [F | f]."""
    F, f = compress_rows(Hc, r)
    return direct(F, f, P, cols, s2)


def information(Hc, r, P, cols, s2):
    """(A Pcc + s^2 I)^-1 [A P[c, :] | b] by a pivoted solve (msckf.hip, "Information form of the stacked update")."""
    Hc, r, P = np.asarray(Hc, float), np.asarray(r, float), np.asarray(P, float)
    A, b = Hc.T @ Hc, Hc.T @ r
    Pc = P[cols, :]
    X = np.linalg.solve(A @ Pc[:, cols] + s2 * np.eye(len(cols)), np.concatenate([A @ Pc, b[:, None]], axis=1))
    Pn = P - Pc.T @ X[:, :-1]
    return Pc.T @ X[:, -1], (Pn + Pn.T) / 2


METHODS = dict(direct=direct, compress=compression, info=information)


# ---- the stacking decisions ---------------------------------------------------------------------------------------------------
def stack_rule(feats, phase, mode=1, kch=KCH):
    """upd_stack_kernel's rule on a stream's candidates (dicts with cams, ok, row) as array arithmetic: a passing feature is stacked if
    the rows stacked BEFORE it are at most 1500 (phase 0; every passing feature in phase 1).
    -> dict(taken: indices, blocks: [(row, len)], m, nc, cols, stacked, path: 'direct' | 'compress' | 'info' | None, mode, kdir)."""
    rows = np.array([4 * len(f['cams']) - 3 for f in feats], dtype=np.int64)
    v = np.where(np.array([bool(f['ok']) for f in feats], dtype=bool), rows, 0) if len(feats) else np.zeros(0, np.int64)
    before = np.cumsum(v) - v
    take = (v > 0) & ((before <= 1500) if phase == 0 else True)
    taken = [int(i) for i in np.flatnonzero(take)]
    used = sorted({int(c) for i in taken for c in feats[i]['cams']})
    cols = np.array([21 + 6 * c + e for c in used for e in range(6)], dtype=np.int64)
    m, nc = int(v[take].sum()), len(cols)
    out = dict(taken=taken, blocks=[(int(feats[i]['row']), int(rows[i])) for i in taken], m=m, nc=nc, cols=cols, path=None, mode=0, kdir=0, stacked=m)
    if mode == 2 or len(taken) > STACK_BLOCKS:
        out.update(m=0, stacked=-1)
        return out
    if m == 0:
        return out
    if phase == 1 and mode == 1 and nc <= INFO_NC and m <= INFO_MAXROWS:
        out.update(path='info', mode=1)
    elif m <= kch:
        out.update(path='direct', kdir=m)
    else:
        out.update(path='compress')
    return out


def reference_loop(feats, cut=True):
    """The reference's own loop (msckf.py:658-668, 759-763): in map order a feature that passes the gate is stacked, and once MORE than
    1500 rows are stacked the loop breaks (the pruning loop has no break).  -> (indices stacked, rows)."""
    k, taken = 0, []
    for i, f in enumerate(feats):
        if f['ok']:
            taken.append(i)
            k += 4 * len(f['cams']) - 3
        if cut and k > 1500:
            break
    return taken, k


def gather(feats, taken, H, r, cols, hld=0):
    """The stacked (Hc, r) of the taken features from a block buffer (H: [rows_cap, ld], or [rows_cap, hld] compact)."""
    idx = np.concatenate([np.arange(feats[i]['row'], feats[i]['row'] + 4 * len(feats[i]['cams']) - 3) for i in taken]) if taken else np.zeros(0, np.int64)
    Hc = H[idx][:, :len(cols)] if hld > 0 else H[idx][:, cols]
    return Hc, r[idx]
