"""Independent pin of rank1_s (csrc/wce_rank1.hip) with a GIVEN w: the branch
`cwg`, where C = u w^T is not Hermitian, g = be^T al is complex and t = q / (b + g)
is a complex division.  No public route reaches that branch with g != 0 (REF,
its only caller, has a = 0), so the arithmetic is pinned on the CPU model
(tests/test_rank1_model.py: model_s(..., cwg=True)) against this file.

    s = (w o x)^T (a diag(x) u w^T diag(x)^H + b I)^-1 rx

evaluated LITERALLY in mpmath at 50 significant digits: the 53 x 53 matrix is
formed by full matrix products and inverted by mpmath's LU inverse; no
Sherman-Morrison, no closed form, nothing from this repository's oracle.
x is the frame's symbol vector with the entries off the mask set to zero (what
State::xmask does in the kernel); rx is used whole.

Frames (numpy RNG, seed below; all inputs are the fp64 values stored here):
  * u = F (conj(F) H_LT / 53), H_LT = rx_pre / tx_pre of inputs.h with the DC
    bin zero, evaluated in mp and rounded to fp64: the TEXTBOOK operating point,
    a = 1, b = ow2 = 9.6172e-8, symbol amplitude 8.8753, cond ~ 4e6;
  * 6 classes x 4 frames: BPSK, QPSK, 16-QAM symbols with a DC null, on the
    preamble's channel ("matched": rx = H_LT x + noise) and on a per-frame
    random channel ("unrelated"); every bit of the mask set;
  * w per class: conj(u) with every entry's phase turned by up to +-0.3 rad and
    its amplitude scaled by up to +-20% -- a non-conjugate vector, g complex;
  * a 7th class with REF's shape: a = 0, b = 2 ow2, the mask holding the four
    pilots only (QPSK, matched).

Output tests/golden/rank1_cw_mp.npz (data only): the fp64 inputs and s as
hi/lo fp64 pairs.  CPU only, about a minute on 8 cores.
Usage: python tests/golden/make_rank1_cw_mp.py
"""
import os
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N = 53
DC = 26
DPS = 50
AMP = 8.8753
SEED = 0xC3A1
PER_CLASS = 4
PILOTS = (5, 19, 33, 47)
CLASSES = [(k, m) for k in ("bpsk", "qpsk", "qam16") for m in (True, False)]


def _mpc(mp, z):
    return mp.mpc(float(z.real), float(z.imag))


def u_vector(tx_pre, rx_pre):
    """u = F ifft(H_LT) in mp, rounded to fp64 (the model and the kernel read fp64)."""
    import mpmath as mp
    mp.mp.dps = DPS
    F = mp.matrix(N, N)
    for t in range(N):
        for f in range(N):
            F[t, f] = mp.expjpi(-2 * mp.mpf(t * f) / N)
    h = mp.matrix(N, 1)
    for k in range(N):
        h[k] = mp.mpc(0) if k == DC else _mpc(mp, rx_pre[k]) / _mpc(mp, tx_pre[k])
    u = F * ((F.transpose_conj() * h) / N)
    hlt = np.array([complex(h[k]) for k in range(N)])
    return np.array([complex(u[k]) for k in range(N)]), hlt


def symbols(rng, kind):
    if kind == "bpsk":
        x = (2.0 * rng.integers(0, 2, N) - 1.0).astype(np.complex128)
    elif kind == "qpsk":
        x = ((2.0 * rng.integers(0, 2, N) - 1) + 1j * (2.0 * rng.integers(0, 2, N) - 1)) / np.sqrt(2.0)
    else:
        lv = np.array([-3.0, -1.0, 1.0, 3.0]) / np.sqrt(10.0)
        x = lv[rng.integers(0, 4, N)] + 1j * lv[rng.integers(0, 4, N)]
    x[DC] = 0.0
    return AMP * x


def frame(rng, kind, matched, hlt, ow2):
    x = symbols(rng, kind)
    if matched:
        h = hlt
    else:
        amp = np.sqrt(np.mean(np.abs(hlt) ** 2) / 2.0)
        h = amp * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    return x, h * x + np.sqrt(ow2 / 2.0) * (rng.standard_normal(N) + 1j * rng.standard_normal(N))


def perturbed_w(rng, u):
    return u.conj() * (1.0 + rng.uniform(-0.2, 0.2, N)) * np.exp(1j * rng.uniform(-0.3, 0.3, N))


def literal_s(args):
    x, rx, u, w, mask, a, b = args
    import mpmath as mp
    mp.mp.dps = DPS
    X = mp.diag([_mpc(mp, x[k]) if mask[k] else mp.mpc(0) for k in range(N)])
    uv = mp.matrix([_mpc(mp, v) for v in u])
    wv = mp.matrix([_mpc(mp, v) for v in w])
    rv = mp.matrix([_mpc(mp, v) for v in rx])
    C = uv * wv.T                                              # u w^T, no conjugate
    Ryy = mp.mpf(float(a)) * (X * C * X.transpose_conj()) + mp.mpf(float(b)) * mp.eye(N)
    z = mp.inverse(Ryy) * rv                                   # LU inverse
    s = ((X * wv).T * z)[0]                                    # (w o x)^T z
    hi = complex(float(s.real), float(s.imag))
    lo = complex(float(s.real - mp.mpf(hi.real)), float(s.imag - mp.mpf(hi.imag)))
    return hi, lo


def main():
    inp = dict(np.load(os.path.join(HERE, "inputs_h.npz")))
    ow2 = float(inp["ow2"])
    u, hlt = u_vector(inp["tx_pre"], inp["rx_pre"])
    rng = np.random.default_rng(SEED)
    tx, rx, ws, masks, ab, cls, names = [], [], [], [], [], [], []
    full = np.ones(N, np.uint8)
    pil = np.zeros(N, np.uint8)
    pil[list(PILOTS)] = 1
    for ci, (kind, matched) in enumerate(CLASSES):
        names.append(f"{kind} {'matched' if matched else 'unrelated'}")
        ws.append(perturbed_w(rng, u))
        for _ in range(PER_CLASS):
            t, r = frame(rng, kind, matched, hlt, ow2)
            tx.append(t); rx.append(r); masks.append(full); ab.append((1.0, ow2)); cls.append(ci)
    names.append("a = 0, pilots (qpsk matched)")
    ws.append(perturbed_w(rng, u))
    for _ in range(PER_CLASS):
        t, r = frame(rng, "qpsk", True, hlt, ow2)
        tx.append(t); rx.append(r); masks.append(pil); ab.append((0.0, 2.0 * ow2)); cls.append(len(CLASSES))
    jobs = [(tx[i], rx[i], u, ws[cls[i]], masks[i], ab[i][0], ab[i][1]) for i in range(len(tx))]
    with Pool(min(8, len(jobs))) as pool:
        res = pool.map(literal_s, jobs)
    out = os.path.join(HERE, "rank1_cw_mp.npz")
    np.savez_compressed(out, tx=np.array(tx), rx=np.array(rx), u=u, w=np.array(ws), mask=np.array(masks),
                        a=np.array([p[0] for p in ab]), b=np.array([p[1] for p in ab]),
                        cls=np.array(cls, np.int64), cls_name=np.array(names),
                        s_hi=np.array([h for h, _ in res]), s_lo=np.array([lo for _, lo in res]),
                        seed=np.int64(SEED), dps=np.int64(DPS))
    print("wrote rank1_cw_mp.npz:", len(tx), "frames,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
