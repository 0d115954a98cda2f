"""Float64 restatement of the silence detector (include/mcvc.h, "silence detection"; librosa.effects.trim / split as published, not verified
against librosa), written from the definition and not from the product code: frame energies from ONE cumulative sum of the squares of the
float32 input, decisions in dB.

    T = 1 + L // 512;   frame t covers samples [512 t - 1024, 512 t + 1024) clipped to [0, L)
    mse[t] = (1 / 2048) sum x^2;   ref = max mse;   db[t] = 10 log10(max(mse[t], 1e-10)) - 10 log10(max(ref, 1e-10))
    frame t is non-silent iff db[t] > -top_db
    trim  = (512 first, min(L, 512 (last + 1)));   split: one such interval per maximal run of non-silent frames
    merge: consecutive intervals whose gap is under round(min_silence_ms * 22.05) samples are joined; then intervals under 16384 samples drop

tests/test_host_silence.py pins the energies to an independent restatement that materialises every frame.  The gates of the GPU tests:

    energy_gate   |mse32 - mse64| <= 1.01 (2048 + 3) 2^-24 mse64 per frame (and for ref): one rounding per square, fewer than 2048 per sum,
                  the scale by 1 / 2048 exact -- it holds for any summation order, with or without FMA.
    band_db       a float32 decision can differ from the float64 one only where db lies within 10 log10((1 + g)^2 (1 + 2^-23)) of -top_db
                  (g: the relative gate above, on mse and on ref; 2^-23: the rounding of r and of the product ref * r).
"""
import numpy as np

FRAME, HOP = 2048, 512
U = 2.0 ** -24                     # unit roundoff of float32
AMIN = 1e-10
MIN_SEGMENT = 16384
G_REL = 1.01 * (FRAME + 3) * U


def frames(L):
    assert L >= 1
    return 1 + L // HOP


def mse(x32):
    """float32 samples -> float64 [T] frame energies."""
    x = np.asarray(x32, dtype=np.float32).reshape(-1).astype(np.float64)
    L = x.size
    c = np.concatenate([[0.0], np.cumsum(x * x)])
    t = np.arange(frames(L), dtype=np.int64)
    lo, hi = np.clip(HOP * t - FRAME // 2, 0, L), np.clip(HOP * t + FRAME // 2, 0, L)
    return (c[hi] - c[lo]) / FRAME


def db(m, ref=None):
    m = np.asarray(m, dtype=np.float64)
    ref = float(m.max()) if ref is None else float(ref)
    return 10.0 * np.log10(np.maximum(m, AMIN)) - 10.0 * np.log10(max(ref, AMIN))


def nonsilent(m, top_db):
    return db(m) > -float(top_db)


def band_db():
    return 10.0 * np.log10((1.0 + G_REL) ** 2 * (1.0 + 2.0 ** -23))


def undecided(m, top_db):
    """-> (frames whose float64 dB lies inside the undecided band around -top_db, distance of the nearest frame to -top_db in dB)."""
    d = np.abs(db(m) + float(top_db))
    return int((d <= band_db()).sum()), float(d.min())


def runs(flags, L):
    """Maximal runs of set flags -> [(start, end)] in samples; asserts order and that none is empty."""
    flags = np.asarray(flags, dtype=bool)
    out, t, T = [], 0, flags.size
    while t < T:
        if flags[t]:
            a = t
            while t + 1 < T and flags[t + 1]:
                t += 1
            out.append((HOP * a, min(L, HOP * (t + 1))))
        t += 1
    last = 0
    for s, e in out:
        assert last <= s < e <= L, (out, L)
        last = e
    return out


def trim(x32, top_db):
    f = np.flatnonzero(nonsilent(mse(x32), top_db))
    L = np.asarray(x32).size
    return int(HOP * f[0]), int(min(L, HOP * (f[-1] + 1)))


def split(x32, top_db):
    return runs(nonsilent(mse(x32), top_db), np.asarray(x32).size)


def merge(intervals, min_silence_ms):
    G = int(round(float(min_silence_ms) * 22.05))
    out = []
    for s, e in intervals:
        if out and s - out[-1][1] < G:
            out[-1] = (out[-1][0], e)
        else:
            out.append((s, e))
    return out


def drop(intervals, min_samples=MIN_SEGMENT):
    kept = [(s, e) for s, e in intervals if e - s >= min_samples]
    return kept, len(intervals) - len(kept)


def split_merged(x32, top_db, min_silence_ms=300.0):
    """-> (kept intervals, number dropped): what SilenceDetector.split returns for one utterance."""
    return drop(merge(split(x32, top_db), min_silence_ms))


def energy_gate(m64):
    return G_REL * np.asarray(m64, dtype=np.float64)


def check_energies(name, got_mse, got_ref, x32):
    """Device energies and maximum (float32) against float64, per element; -> the largest error / gate."""
    want = mse(x32)
    got_mse = np.asarray(got_mse)
    assert got_mse.dtype == np.float32 and got_mse.shape == want.shape, (name, got_mse.dtype, got_mse.shape, want.shape)
    assert np.asarray(got_ref).dtype == np.float32
    err = np.concatenate([np.abs(got_mse.astype(np.float64) - want), [abs(float(got_ref) - float(want.max()))]])
    g = np.concatenate([energy_gate(want), [energy_gate(want.max())]])
    worst = float(np.max(np.where(err > 0, err / np.maximum(g, 1e-300), 0.0)))
    print("%s: %d samples, %d frames  max err %.3e  worst err / gate %.3f" % (name, np.asarray(x32).size, want.size, float(err.max()), worst))
    assert (err <= g).all(), (name, worst)
    return worst


def assert_decidable(name, x32, top_db):
    """No frame of this input may lie in the undecided band: an ill-chosen input fails here, loudly, before anything is compared."""
    n, nearest = undecided(mse(x32), top_db)
    print("%s at %g dB: nearest frame %.4f dB from the threshold (band %.2e dB)" % (name, top_db, nearest, band_db()))
    assert n == 0, "%s: %d frames within %.2e dB of -%g dB: choose another input" % (name, n, band_db(), top_db)
    return nearest
