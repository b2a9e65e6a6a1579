"""Framing the payload, the parts that need no GPU: the entry points exist (libwce.so, include/wce.h,
the Python mirrors and their keywords), every refusal of the header is made before the context is
touched, and the numpy model (tests/psdu_model.py) that the GPU tests hold the kernel to is itself held
to the standard's published vectors: the 127-bit sequence of seed 127, the opening of the worked example's
seed 93, CRC-32's check value and its residue."""
import ctypes
import inspect
import os
import re
import zlib

import numpy as np
import pytest

import psdu_model as pm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
SEQ_127 = ("00001110 11110010 11001001 00000010 00100110 00101110 10110110 00001100 11010100 11100111 10110100 "
           "00101010 11111010 01010001 10111000 1111111").replace(" ", "")


# ---------------------------------------------------------------- 1. the interface
def test_symbols_exported_and_declared(wce):
    lib = wce.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "wce.h")).read(), flags=re.S)
    for name, nargs in (("wce_psdu_max_len", 2), ("wce_psdu_frame", 8), ("wce_psdu_deframe", 7)):
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1).split(",")
        assert len(params) == len(wce.wce.ABI[name]) == nargs, name
    W = wce.wce
    assert [f[0] for f in W.PsduPar._fields_] == ["modulation", "rate", "length", "seed", "lengths", "seeds"]
    assert [f[0] for f in W.PsduOut._fields_] == ["psdu", "psdu_stride", "seed", "fcs_ok", "n_good"]
    assert ctypes.sizeof(W.PsduPar) == 32 and ctypes.sizeof(W.PsduOut) == 40
    for struct, cls in (("wce_psdu_par", W.PsduPar), ("wce_psdu_out", W.PsduOut)):
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % struct, hdr)
        assert body, struct
        assert re.findall(r"\b(\w+)\s*(?=[,;])", body.group(1)) == [f[0] for f in cls._fields_], struct
    assert wce.PsduPar is W.PsduPar and wce.PsduOut is W.PsduOut and wce.psdu_max_len is W.psdu_max_len


def test_python_keywords(wce):
    C = wce.Context
    for fn, kws in ((C.psdu_frame, {"length": None, "lengths": None, "seed": 93, "seeds": None, "bits": None,
                                    "payload_stride": None, "bits_stride": None, "stream": None}),
                    (C.psdu_deframe, {"length": None, "lengths": None, "psdu": None, "seed": None, "fcs_ok": None,
                                      "n_good": None, "bits_stride": None, "psdu_stride": None, "stream": None}),
                    (C.psdu_frame_host, {"seeds": 93}),
                    (C.link_host, {"psdu_len": None}), (C.link_mrc_host, {"psdu_len": None})):
        p = inspect.signature(fn).parameters
        for k, default in kws.items():
            assert k in p and p[k].default == default, (fn.__name__, k)
    assert list(inspect.signature(C.psdu_frame).parameters)[1:5] == ["payload", "n_frames", "modulation", "rate"]
    assert list(inspect.signature(C.psdu_deframe).parameters)[1:5] == ["bits", "n_frames", "modulation", "rate"]
    assert list(inspect.signature(C.psdu_frame_host).parameters)[1:4] == ["payloads", "modulation", "rate"]
    assert list(inspect.signature(C.psdu_deframe_host).parameters)[1:] == ["bits", "modulation", "rate", "lengths"]


def test_max_len(wce):
    lib = wce.load()
    seen = set()
    for mod, rate in pm.PAIRS:
        T = wce.info_bits(mod, rate)
        assert T == pm.info_bits(mod, rate)
        assert wce.psdu_max_len(mod, rate) == lib.wce_psdu_max_len(mod, rate) == (T - 22) // 8 == pm.max_len(mod, rate)
        # there always are pad bits, and the tail's byte is inside the row
        assert (T - 22) % 8 == (6 if T == 540 else 2) and pm.max_len(mod, rate) + 3 <= pm.nbytes(mod, rate)
        seen.add(T)
    assert min(seen) == 360 and max(seen) == 3240
    assert wce.psdu_max_len(wce.MOD_BPSK, wce.RATE_1_2) == 42 and wce.psdu_max_len(wce.MOD_QAM64, wce.RATE_3_4) == 402
    for mod, rate in ((3, 0), (0, 0), (1, 3), (1, -1)):
        assert lib.wce_psdu_max_len(mod, rate) == EINVAL and "unknown modulation or rate" in lib.wce_last_error().decode()
        with pytest.raises(wce.WceError):
            wce.psdu_max_len(mod, rate)


# ---------------------------------------------------------------- 2. the refusals
# QPSK 1/2: T = 720, 90 bytes a row, max = 87
MOD, RATE, NBYTES, MAX = 2, 0, 90, 87


def _base():
    par = dict(modulation=MOD, rate=RATE, length=40, seed=93, lengths=None, seeds=None)
    frame = dict(payload=0x1001, payload_stride=36, n_frames=3, bits=0x2001, bits_stride=NBYTES)
    out = dict(psdu=0x3001, psdu_stride=40, seed=0x4001, fcs_ok=0x5000, n_good=0x6000)
    return par, frame, out


def _frame(wce, lib, ctx, par, fr):
    p = wce.wce.PsduPar(**par) if par is not None else None
    return lib.wce_psdu_frame(ctx, ctypes.byref(p) if p is not None else None, fr["payload"], fr["payload_stride"],
                              fr["n_frames"], fr["bits"], fr["bits_stride"], None)


def _deframe(wce, lib, ctx, par, fr, out):
    p = wce.wce.PsduPar(**par) if par is not None else None
    o = wce.wce.PsduOut(**out) if out is not None else None
    return lib.wce_psdu_deframe(ctx, ctypes.byref(p) if p is not None else None, fr["bits"], fr["bits_stride"],
                                fr["n_frames"], ctypes.byref(o) if o is not None else None, None)


BOTH_REFUSALS = [
    ({"modulation": 3}, {}, "unknown modulation or rate"), ({"modulation": 0}, {}, "unknown modulation or rate"),
    ({"rate": 3}, {}, "unknown modulation or rate"), ({"rate": -1}, {}, "unknown modulation or rate"),
    ({"length": 3}, {}, "length outside"), ({"length": MAX + 1}, {}, "length outside"),
    ({}, {"bits_stride": NBYTES - 1}, "bits_stride"), ({}, {"bits": None}, "null"),
    ({"lengths": 0x7002}, {}, "lengths not 4-byte aligned"),
    ({}, {"n_frames": -1}, "n_frames"), ({}, {"n_frames": 2 ** 31}, "n_frames"),
]
FRAME_REFUSALS = [
    ({"seed": 0}, {}, "seed outside"), ({"seed": 128}, {}, "seed outside"),
    ({}, {"payload": None}, "payload NULL"), ({"length": 5}, {"payload": None}, "payload NULL"),
    ({"lengths": 0x7000, "length": 4}, {"payload": None, "payload_stride": MAX - 4}, "payload NULL"),
    ({}, {"payload_stride": 35}, "payload_stride"),
    ({"lengths": 0x7000}, {"payload_stride": MAX - 5}, "payload_stride"),
]
DEFRAME_REFUSALS = [
    ({}, {"psdu": None, "seed": None, "fcs_ok": None, "n_good": None}, "no output"),
    ({}, {"psdu_stride": 39}, "psdu_stride"), ({"lengths": 0x7000}, {"psdu_stride": MAX - 1}, "psdu_stride"),
    ({}, {"fcs_ok": 0x5002}, "4-byte"), ({}, {"n_good": 0x6001}, "4-byte"),
]


def test_refusals_before_the_ctx_is_touched(wce):
    """every WCE_EINVAL of the header, with an opaque non-NULL ctx and opaque pointers: nothing is launched.  The
    calls that hold are made with n_frames = 0, which returns WCE_OK after the same validation."""
    lib = wce.load()
    ctx = 0x10
    for pch, fch, text in BOTH_REFUSALS + FRAME_REFUSALS:
        par, fr, out = _base()
        assert _frame(wce, lib, ctx, {**par, **pch}, {**fr, **fch}) == EINVAL, (pch, fch)
        assert text in lib.wce_last_error().decode() and "wce_psdu_frame" in lib.wce_last_error().decode(), (pch, fch)
    for pch, fch, text in BOTH_REFUSALS:
        par, fr, out = _base()
        assert _deframe(wce, lib, ctx, {**par, **pch}, {**fr, **fch}, out) == EINVAL, (pch, fch)
        assert text in lib.wce_last_error().decode() and "wce_psdu_deframe" in lib.wce_last_error().decode(), (pch, fch)
    for pch, och, text in DEFRAME_REFUSALS:
        par, fr, out = _base()
        assert _deframe(wce, lib, ctx, {**par, **pch}, fr, {**out, **och}) == EINVAL, (pch, och)
        assert text in lib.wce_last_error().decode(), (pch, och, lib.wce_last_error())
    par, fr, out = _base()
    assert _frame(wce, lib, None, par, fr) == EINVAL and "null ctx" in lib.wce_last_error().decode()
    assert _deframe(wce, lib, None, par, fr, out) == EINVAL and "null ctx" in lib.wce_last_error().decode()
    assert _frame(wce, lib, ctx, None, fr) == EINVAL and _deframe(wce, lib, ctx, None, fr, out) == EINVAL
    assert _deframe(wce, lib, ctx, par, fr, None) == EINVAL
    # what holds: n_frames = 0 after the same validation
    zero = {**fr, "n_frames": 0}
    assert _frame(wce, lib, ctx, par, zero) == 0 and _deframe(wce, lib, ctx, par, zero, out) == 0
    # L = 4 needs no payload; lengths and seeds replace length and seed, whatever those hold; deframing ignores the
    # seed; each output alone is enough; the limits themselves are in range
    assert _frame(wce, lib, ctx, {**par, "length": 4}, {**zero, "payload": None, "payload_stride": 0}) == 0
    assert _frame(wce, lib, ctx, {**par, "lengths": 0x7000, "length": 0}, {**zero, "payload_stride": MAX - 4}) == 0
    assert _frame(wce, lib, ctx, {**par, "seeds": 0x7001, "seed": 0}, zero) == 0
    assert _frame(wce, lib, ctx, {**par, "length": MAX, "seed": 127}, {**zero, "payload_stride": MAX - 4}) == 0
    assert _frame(wce, lib, ctx, {**par, "length": 4, "seed": 1}, {**zero, "payload_stride": 0}) == 0
    assert _deframe(wce, lib, ctx, {**par, "seed": 0, "seeds": 0x7003}, zero, out) == 0
    assert _deframe(wce, lib, ctx, {**par, "lengths": 0x7000, "length": 0}, zero, {**out, "psdu_stride": MAX}) == 0
    none = dict(psdu=None, psdu_stride=0, seed=None, fcs_ok=None, n_good=None)
    for k in ("psdu", "seed", "fcs_ok", "n_good"):
        one = {**none, k: out[k], "psdu_stride": 40}
        assert _deframe(wce, lib, ctx, par, zero, one) == 0, k
    assert _deframe(wce, lib, ctx, par, zero, {**out, "psdu": None, "psdu_stride": 0}) == 0


def test_link_host_default_and_refusal(wce):
    assert inspect.signature(wce.Context.link_host).parameters["psdu_len"].default is None
    assert inspect.signature(wce.Context.link_mrc_host).parameters["psdu_len"].default is None
    c = object.__new__(wce.Context)
    c.handle, c.tx_pre = None, None
    for L in (3, 88, -1):
        with pytest.raises(ValueError, match="psdu_len"):
            c.link_host(MOD, RATE, 30.0, 2, psdu_len=L)
        with pytest.raises(ValueError, match="psdu_len"):
            c.link_mrc_host(MOD, RATE, 30.0, 2, 2, np.ones((2, 6)) / 6, psdu_len=L)


# ---------------------------------------------------------------- 3. the model against the standard
def test_scrambler_vectors():
    assert "".join(map(str, pm.scrambler(127, 127))) == SEQ_127
    assert "".join(map(str, pm.scrambler(93, 16))) == "0110110000011001"
    for seed in (1, 93, 127):
        s = pm.scrambler(seed, 300)
        assert np.array_equal(s[7:], s[3:-4] ^ s[:-7]) and np.array_equal(s[127:], s[:-127])
    # every seed is the seed-127 sequence at a phase of its own, and seven bits name the seed
    two = "".join(map(str, pm.scrambler(127, 254)))
    phases = {two.index("".join(map(str, pm.scrambler(seed, 127)))) for seed in range(1, 128)}
    assert phases == set(range(127))
    assert [pm.seed_of(pm.scrambler(seed, 7)) for seed in range(1, 128)] == list(range(1, 128))
    assert pm.seed_of(np.zeros(7, np.uint8)) == 0


def test_crc_vectors():
    assert zlib.crc32(b"123456789") == 0xCBF43926
    assert bytes(pm.fcs(np.frombuffer(b"123456789", np.uint8))) == bytes([0x26, 0x39, 0xF4, 0xCB])
    rng = np.random.default_rng(5)
    for n in (0, 1, 3, 4, 5, 38, 398):
        assert zlib.crc32(bytes(pm.psdu_of(rng.integers(0, 256, n).astype(np.uint8)))) == pm.RESIDUE == 0x2144DF1C


@pytest.mark.parametrize("mod,rate", pm.PAIRS)
def test_model_round_trip(mod, rate):
    T, mx = pm.info_bits(mod, rate), pm.max_len(mod, rate)
    rng = np.random.default_rng(100 * mod + rate)
    for L in (4, 5, mx):
        payload = rng.integers(0, 256, L - 4).astype(np.uint8)
        seed = int(rng.integers(1, 128))
        bits = pm.frame_one(payload, seed, T)
        assert bits.shape == (T,) and not bits[16 + 8 * L:16 + 8 * L + 6].any()          # the tail is 0 on the air
        assert np.array_equal(bits[:7], pm.scrambler(seed, 7))                            # SERVICE shows the seed
        assert np.array_equal(bits[16 + 8 * L + 6:], pm.scrambler(seed, T)[16 + 8 * L + 6:])   # the pad is scrambled 0
        psdu, got_seed, ok = pm.deframe_one(bits, L, T)
        assert ok == 1 and got_seed == seed and np.array_equal(psdu[:L - 4], payload)
        assert np.array_equal(psdu, pm.psdu_of(payload))
        # one bit anywhere in the PSDU loses the frame; the tail and the pad do not count
        for t, want in ((16, 0), (16 + 8 * L - 1, 0), (16 + 8 * L, 1), (T - 1, 1), (7, 1), (15, 1), (0, 0)):
            bad = bits.copy()
            bad[t] ^= 1
            assert pm.deframe_one(bad, L, T)[2] == want, (L, t)
    assert not pm.frame_one(np.zeros(mx - 3, np.uint8), 93, T).any() and not pm.frame_one(np.zeros(0, np.uint8), 0, T).any()
    assert pm.deframe_one(np.ones(T, np.uint8), 3, T) == (None, 0, 0) and pm.deframe_one(np.ones(T, np.uint8), mx + 1, T)[0] is None
    z = pm.deframe_one(np.zeros(T, np.uint8), mx, T)
    assert z[1] == 0 and z[2] == 0 and not z[0].any()
    assert np.array_equal(pm.unpack(pm.pack(bits), T), bits) and pm.pack(bits).size == pm.nbytes(mod, rate)


# ---------------------------------------------------------------- 4. the link experiment's low SNR
def test_link_snr_was_chosen_on_the_model():
    """tests/test_psdu_gpu.py asks of the device that LT_LS leaves at least 5 good and at least 5 bad packets of 67
    at LINK_SNR_LOW: the numpy chain says 33 and 34 there, and none bad at LINK_SNR_HIGH"""
    low = pm.link_model(pm.LINK_SNR_LOW)
    good = int(low["fcs_ok"].sum())
    print(f"{pm.LINK_SNR_LOW} dB: detected {int(low['detected'].sum())}, good {good}, bad {pm.LINK_B - good}")
    assert (good, pm.LINK_B - good) == (33, 34) and low["detected"].all()
    c = pm.link_set()
    rx = [pm.deframe_one(b, c["L"], b.size) for b in low["bits"]]
    sent = np.array([np.array_equal(r[0], pm.psdu_of(p)) and r[1] == s for r, p, s in zip(rx, c["payload"], c["seeds"])])
    assert np.array_equal(sent, low["fcs_ok"] == 1)           # no CRC miss, and no good frame with a wrong PSDU
    # the FCS sits next to the unterminated end: how many packets lose it alone (a figure, nothing is asked of it)
    print("payload right, FCS wrong:", sum(np.array_equal(r[0][:-4], p) and not ok
                                            for r, p, ok in zip(rx, c["payload"], sent)))
    high = pm.link_model(pm.LINK_SNR_HIGH)
    assert high["detected"].all() and high["fcs_ok"].all() and np.array_equal(high["bits"][:, :16 + 8 * c["L"]], c["bits"][:, :16 + 8 * c["L"]])
