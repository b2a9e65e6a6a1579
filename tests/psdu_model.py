"""numpy model of the DATA-field framing (wce_psdu_frame / wce_psdu_deframe, include/wce.h): 802.11's
scrambler by its state machine, one bit per step, the field layout, and the FCS from zlib.crc32.  It shares
no table and no trick with the kernel (csrc/wce_psdu.hip), which never steps the scrambler and never runs a
CRC over more than eight octets.

Bits are one per uint8 entry, [B][T] with T = info_bits(modulation, rate); pack() / unpack() go to and from
the rows the library reads and writes (LSB first)."""
import zlib

import numpy as np

import fec_model as fm

RESIDUE = 0x2144DF1C          # crc32 over a PSDU with its FCS
SERVICE = 16
PAIRS = [(m, r) for m in (1, 2, 4, 6) for r in (fm.RATE_1_2, fm.RATE_2_3, fm.RATE_3_4)]


def info_bits(mod, rate):
    return fm.info_bits(mod, rate)


def max_len(mod, rate):
    return (info_bits(mod, rate) - 22) // 8


def nbytes(mod, rate):
    return (info_bits(mod, rate) + 7) // 8


def scrambler(seed, n):
    """n outputs of x^7 + x^4 + 1 from the state whose x_i is bit i - 1 of seed"""
    x = [(seed >> i) & 1 for i in range(7)]     # x[0] = x1 .. x[6] = x7
    out = np.empty(n, np.uint8)
    for t in range(n):
        s = x[3] ^ x[6]
        out[t] = s
        x = [s] + x[:6]
    return out


def seed_of(first7):
    """the initial state that sends the seven bits s_0..s_6, 0 if they are all 0"""
    first7 = [int(b) for b in first7]
    if not any(first7):
        return 0
    for seed in range(1, 128):
        if list(scrambler(seed, 7)) == first7:
            return seed
    raise AssertionError("no seed")


def fcs(octets):
    return np.frombuffer(int(zlib.crc32(bytes(octets)) & 0xFFFFFFFF).to_bytes(4, "little"), np.uint8)


def psdu_of(payload):
    payload = np.asarray(payload, np.uint8)
    return np.concatenate([payload, fcs(payload)])


def frame_one(payload, seed, T):
    """payload (L - 4 octets) -> the T framed, scrambled bits; an L or a seed out of range -> zeros"""
    payload = np.asarray(payload, np.uint8)
    L = payload.size + 4
    if not (4 <= L <= (T - 22) // 8 and 1 <= seed <= 127):
        return np.zeros(T, np.uint8)
    field = np.zeros(T, np.uint8)
    field[SERVICE:SERVICE + 8 * L] = np.unpackbits(psdu_of(payload), bitorder="little")
    out = field ^ scrambler(seed, T)
    out[SERVICE + 8 * L:SERVICE + 8 * L + 6] = 0
    return out


def frame(payloads, seeds, mod, rate):
    T = info_bits(mod, rate)
    return np.stack([frame_one(p, int(s), T) for p, s in zip(payloads, seeds)])


def deframe_one(bits, L, T):
    """-> (psdu octets or None where nothing is written, seed, fcs_ok)"""
    if not 4 <= L <= (T - 22) // 8:
        return None, 0, 0
    seed = seed_of(bits[:7])
    d = np.asarray(bits, np.uint8) ^ scrambler(seed, T) if seed else np.asarray(bits, np.uint8)
    psdu = np.packbits(d[SERVICE:SERVICE + 8 * L], bitorder="little")
    ok = int(seed != 0 and (zlib.crc32(bytes(psdu)) & 0xFFFFFFFF) == RESIDUE)
    return psdu, seed, ok


def deframe(bits, lengths, mod, rate):
    """bits [B][T], lengths [B] -> (list of psdu rows or None, seed uint8 [B], fcs_ok uint32 [B])"""
    T = info_bits(mod, rate)
    res = [deframe_one(b, int(L), T) for b, L in zip(bits, lengths)]
    return [r[0] for r in res], np.array([r[1] for r in res], np.uint8), np.array([r[2] for r in res], np.uint32)


def pack(bits):
    return np.packbits(np.asarray(bits, np.uint8), axis=-1, bitorder="little")


def unpack(rows, T):
    return np.unpackbits(np.asarray(rows, np.uint8), axis=-1, bitorder="little")[..., :T]


# ---- the link experiment of tests/test_psdu_gpu.py, on the numpy chain models
LINK_MOD, LINK_RATE, LINK_B = 2, fm.RATE_1_2, 67
LINK_SEED = 0x80211            # link_host's default: payload, scrambler seeds and the noise
LINK_TAPS_SEED = 0x7A95
# 10 dB less per tap: link_host's sources include PS_LINEAR, which draws straight lines between pilots 14 bins
# apart.  A tap at delay d turns by 2 pi 14 d / 64 = 1.37 d rad from pilot to pilot, so the chord misses it by up to
# 1 - cos(0.69 d) of its size: 0.23, 0.80 and about 1.5 for d = 1, 2, 3.  With powers 1e-1, 1e-2, 1e-3 that is an error
# floor near 0.1 0.05 + 0.01 0.64 + 0.001 2.2 = 0.014 of the channel's power, -18 dB, which rate-1/2 QPSK decodes
# through; a profile that decays by e^-1/2 a tap would leave it -6 dB and PS_LINEAR with bit errors at any SNR
LINK_POWER = 10.0 ** -np.arange(6.0)
LINK_LEN, LINK_THRESHOLD = 1488, 0.25
LINK_SNR_HIGH = 30.0
# chosen here, on the CPU, before the device saw it: pdp_taps gives every packet unit channel energy and this profile
# is close to flat, so the packets share one SNR and the step from all bad to all good is narrow.  The model below
# detects all 67 packets and LT_LS leaves 20 good / 47 bad at 4 dB, 33 / 34 at 4.5 dB, 46 / 21 at 5 dB, 58 / 9 at 6 dB
# and 67 / 0 at 8 dB: 4.5 dB keeps both kinds far from the 5 the test asks for
LINK_SNR_LOW = 4.5


def link_set():
    """link_host(psdu_len = max)'s own draws from LINK_SEED, and the taps -> dict"""
    import fading_model as fd
    L = max_len(LINK_MOD, LINK_RATE)
    rng = np.random.default_rng(LINK_SEED)
    payload = rng.integers(0, 256, (LINK_B, L - 4)).astype(np.uint8)
    seeds = rng.integers(1, 128, LINK_B).astype(np.uint8)
    return {"L": L, "payload": payload, "seeds": seeds, "bits": frame(payload, seeds, LINK_MOD, LINK_RATE),
            "taps": fd.pdp_taps(np.random.default_rng(LINK_TAPS_SEED), LINK_B, LINK_POWER)}


def link_model(snr_db, real=np.float64):
    """the packets of link_set through tx_model's transmitter and channel at nominal snr_db and the numpy receive
    chain with LT_LS (sync, the two-copy offset estimate, tracked demodulation, soft bits, the unterminated
    decoder), then deframe_one -> dict detected [B] bool, bits [B][T] (zeros where undetected), fcs_ok [B]"""
    import cfo_model as cm
    import demod_model as dm
    import sync_model as sm
    import tx_model as tm
    c = link_set()
    mod, rate, B = LINK_MOD, LINK_RATE, LINK_B
    T = info_bits(mod, rate)
    pre = tm.chain_pre()
    tx = fm.transmit(c["bits"], mod, rate)[0]
    cap = np.asarray(tm.transmit(tx, LINK_LEN, pre, real, taps=c["taps"],
                                 ow2=np.full(B, float(tm.nominal_ow2(snr_db))), seed=LINK_SEED), np.complex128)
    ltf = np.asarray(tm.idft64(pre, tm.LD), np.complex128)
    start = sm.sync(cap, ltf, LINK_THRESHOLD, 0, real)[0]
    det = np.array([0 <= s and s + 1328 <= LINK_LEN for s in start])
    idx = np.flatnonzero(det)
    field = np.stack([cap[f, start[f]:start[f] + 128] for f in idx])
    pk = np.stack([cap[f, start[f] + 128:start[f] + 1328] for f in idx])
    eps = np.asarray(cm.estimate(field, real), np.float64)
    rx_pre, _ = cm.preamble(field, eps, real)
    rx = cm.blocks(pk, eps, 0, 15, real)
    with np.errstate(invalid="ignore", divide="ignore"):      # DC: 0 / 0, then set to 0
        h = dm.lt_ls(np.broadcast_to(pre, (len(idx), 53)), rx_pre, real)
    d = dm.demodulate(tx[idx], rx, h, None, mod, tm.SCALE, True, True, real)
    bits = np.zeros((B, T), np.uint8)
    bits[idx] = fm.decode(fm.llr(d["eq"], dm.blend(h, None, real), mod, tm.SCALE, real), mod, rate, terminated=False)
    return {"detected": det, "bits": bits, "fcs_ok": deframe(bits, np.full(B, c["L"]), mod, rate)[2]}
