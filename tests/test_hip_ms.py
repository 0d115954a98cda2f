"""GPU checks of the modulation-spectrum kernels (csrc/ms_kernels.hip through mask_cyclegan_vc/metrics.py and the evaluate CLI) against the
float64 restatement tests/ms_checker.py.

Shapes: K = 1 (all but one row of a tile padded), 24 (the default), 33 (one row into the second tile), 80 (the limit, three tiles);
T = 1, 2, 3, one short of / exactly / one past a staged chunk of 64, three chunks with a ragged end (130), eleven (700), and T = n_fft;
n_fft = 1024, 2048, 4096.  Trajectories: a seeded random walk plus white noise, 0.1 cumsum(N(0, 1)) + 0.05 N(0, 1).

The gates are derived from the kernel's chain lengths, not measured.  u = 2^-24 (unit roundoff), nc = ceil(T / 64) (staged chunks = lane
chain of the row sums), x the checker's float64 deviations, c the input row.

x.  The kernel forms m0 = fl(sum c / T), r = fl(sum fl(c - m0) / T), x^ = fl(fl(c - m0) - r).  A row sum is a lane chain of nc additions,
    six butterfly levels and a division: relative error (nc + 7) u of sum |terms|.  So |m0 - mean| <= (nc + 7) u sum|c| / T =: rb, the
    correction r is known to dr = (nc + 8) u (sum|x| / T + rb), and |x^_t - x_t| <= 2 u |x_t| + E with E = 2 u rb + dr.  Summed over t:
    sum_t |x^_t - x_t| <= (nc + 10) u sum|x| + (nc + 10)(nc + 7) u^2 sum|c|.  The last term is second order; the tests assert
    sum|c| <= 1000 sum|x| for their rows, which makes it at most 0.4 u sum|x| (nc <= 64): one more unit of C below.
X.  Each twiddle is a float64 value rounded once (<= u / 2 absolute per component); a chunk is a fused chain of at most 64 terms summed
    from zero, the chunks a chain of nc additions: per component (64 + nc + 1) u sum|x|, for the complex value sqrt(2) times that.
P.  P = fl(fl(re^2 + im^2) / T): three roundings, 1.5 u |X|^2 / T <= (2 |X| / T)(0.75 u sum|x|): one more unit of C.
    Together |X^ - X| <= delta = C 2^-24 sum_t |x_t| with C = sqrt(2) (65 + nc) + nc + 12, and |P - P64| <= (2 |X64| delta + delta^2) / T.
    (C = 106 at T = 64, 258 at T = 4096; the straight float32 matrix DFT the issue measured sat at 9.)
mean.  |mean - mean64| <= u |mean64| + dr (the final addition, the correction).
var.   var = fl(sum x^^2 / T), a positive chain: relative (nc + 8) u, plus the error of x^: 2 sum |x| e + sum e^2 with e = 2 u |x| + E.

Exact bin placement: the issue asks for a peak of T / 4 at bins 1, 1000 and 2048 of n_fft = 4096 and at bin 512 of n_fft = 1024.  At the
Nyquist bin (2048 of 4096, 512 of 1024) a unit cosine is (-1)^t, X = T and the peak is T, not T / 4 (tests/test_host_ms.py checks the
fact on the checker); the test takes T / 4 below Nyquist and T at Nyquist, with the gate of P and the same 1e-6 T / 4 for all other bins.

Largest observed figures on an MI355X (profiles/ms_error.json): |dP| / bound 0.057, |dmean| / bound 0.74, |dvar| / bound 0.11,
|d dB| 8.2e-3 dB over the utterances of T >= 63 (the issue's CPU estimate for a straight matrix DFT on its own data: 2.4e-3 dB)."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ms_checker as ck  # noqa: E402
from mask_cyclegan_vc import _hip, evaluate, metrics  # noqa: E402

U = 2.0 ** -24
TS = (1, 2, 3, 63, 64, 65, 130, 700)
KS = (1, 24, 33, 80)
COMBOS = [(K, n_fft) for K in KS for n_fft in ck.FFTS]
GUARD = 64
MCVC_ERR_INVALID = 1001
WORST = {"dP_over_bound": 0.0, "ddB": 0.0, "dmean_over_bound": 0.0, "dvar_over_bound": 0.0}


def nchunks(T):
    return (T + 63) // 64


def c_of(T):
    return math.sqrt(2.0) * (65 + nchunks(T)) + nchunks(T) + 12


def bounds(c, n_fft):
    """float32 [K, T] -> dict of float64 references and derived gates (module docstring)."""
    X, x, mean, var = ck.spectrum(c, n_fft)
    K, T = x.shape
    nc = nchunks(T)
    sx, sc, s2 = np.abs(x).sum(axis=1), np.abs(np.asarray(c, dtype=np.float64)).sum(axis=1), (x * x).sum(axis=1)
    assert (sc <= 1000.0 * sx)[sx > 0].all()                                  # the precondition of the second-order term
    delta = c_of(T) * U * sx
    absX = np.abs(X)
    P = (X.real ** 2 + X.imag ** 2) / T
    rb = (nc + 7) * U * sc / T
    dr = (nc + 8) * U * (sx / T + rb) * 1.01
    E = 2 * U * rb + dr
    zero = sx == 0                                                            # a constant row: every quantity is exact
    b_mean = np.where(zero, 0.0, U * np.abs(mean) + dr)
    b_var = np.where(zero, 0.0, ((nc + 8 + 4) * U * s2 + 2 * E * sx + 8 * U * U * s2 + 2 * T * E * E) / T * 1.01)
    return {"P": P, "absX": absX, "mean": mean, "var": var, "delta": delta, "b_P": (2 * absX * delta[:, None] + delta[:, None] ** 2) / T,
            "b_mean": b_mean, "b_var": b_var, "T": T, "sx": sx}


def make(K, n_fft):
    rs = np.random.RandomState(100 * K + n_fft // 1024)
    return [ck.trajectory(rs, K, T) for T in TS + (n_fft,)]


@pytest.fixture(scope="module")
def data():
    return {combo: make(*combo) for combo in COMBOS}


@pytest.fixture(scope="module")
def want(data):
    """float64 references and gates on the same float32 trajectories, computed once."""
    return {combo: [bounds(c, combo[1]) for c in data[combo]] for combo in COMBOS}


def raw_power(utts, n_fft, fill=float("nan")):
    """The C ABI with buffers of this test's own: outputs pre-filled with NaN, GUARD elements on both sides.  -> (P, mean, var) numpy per bank,
    after checking that every element was written and no guard was touched."""
    L = _hip.lib()
    b, offs = metrics.bank(utts)
    K, n = b.shape[0], len(utts)
    table = _hip.device_constant(("metrics.ms_table", n_fft), b.device, lambda: metrics.host_ms_table(n_fft))
    offs_d = torch.from_numpy(offs).cuda()
    sizes = {"power": n * K * (n_fft // 2), "mean": n * K, "var": n * K}
    bufs = {k: torch.full((v + 2 * GUARD,), fill, dtype=torch.float32, device="cuda") for k, v in sizes.items()}
    inner = {k: bufs[k][GUARD:GUARD + v] for k, v in sizes.items()}
    rc = L.mcvc_ms_power(_hip.ptr(b), b.shape[1], K, _hip.ptr(offs_d), n, offs.ctypes.data, n_fft, _hip.ptr(table), _hip.ptr(inner["power"]),
                         _hip.ptr(inner["mean"]), _hip.ptr(inner["var"]), _hip.stream())
    assert rc == 0
    torch.cuda.synchronize()
    out = {}
    for k, v in sizes.items():
        host = bufs[k].cpu().numpy()
        assert np.isnan(host[:GUARD]).all() and np.isnan(host[GUARD + v:]).all(), "%s: a guard element was written" % k
        assert not np.isnan(host[GUARD:GUARD + v]).any(), "%s: an element was not written" % k
        out[k] = host[GUARD:GUARD + v]
    return out["power"].reshape(n, K, n_fft // 2), out["mean"].reshape(n, K), out["var"].reshape(n, K)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check_against(P, mean, var, w, tag):
    P, mean, var = P.astype(np.float64), mean.astype(np.float64), var.astype(np.float64)
    eP, em, ev = np.abs(P - w["P"]), np.abs(mean - w["mean"]), np.abs(var - w["var"])
    rP = float(np.max(np.where(w["b_P"] > 0, eP / np.where(w["b_P"] > 0, w["b_P"], 1.0), 0.0)))
    rm = float(np.max(np.where(w["b_mean"] > 0, em / np.where(w["b_mean"] > 0, w["b_mean"], 1.0), 0.0)))
    rv = float(np.max(np.where(w["b_var"] > 0, ev / np.where(w["b_var"] > 0, w["b_var"], 1.0), 0.0)))
    ddb = 0.0
    if w["T"] >= 63:
        ddb = float(np.abs(10.0 * np.log10(np.maximum(P, ck.FLOOR)) - 10.0 * np.log10(np.maximum(w["P"], ck.FLOOR))).max())
    print("%s T=%d: |dP|/bound %.4f (C = %.0f), |dmean|/bound %.4f, |dvar|/bound %.4f, |d dB| %.2e" % (tag, w["T"], rP, c_of(w["T"]), rm, rv, ddb))
    WORST["dP_over_bound"] = max(WORST["dP_over_bound"], rP)
    WORST["dmean_over_bound"] = max(WORST["dmean_over_bound"], rm)
    WORST["dvar_over_bound"] = max(WORST["dvar_over_bound"], rv)
    WORST["ddB"] = max(WORST["ddB"], ddb)
    assert (eP <= w["b_P"]).all() and (em <= w["b_mean"]).all() and (ev <= w["b_var"]).all(), tag


# ---- 1. element by element against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n_fft", COMBOS)
def test_power_mean_var_against_float64(data, want, K, n_fft):
    utts = data[(K, n_fft)]
    P, mean, var = raw_power(utts, n_fft)
    for i, w in enumerate(want[(K, n_fft)]):
        check_against(P[i], mean[i], var[i], w, "K=%d n_fft=%d" % (K, n_fft))
    path = os.environ.get("MCVC_MS_ERROR_JSON")
    if path:                                                                  # (how profiles/ms_error.json was recorded)
        with open(path, "w") as fh:
            json.dump(dict(WORST, note="largest over the cases of test_power_mean_var_against_float64 run so far"), fh, indent=1)


# ---- 2. exact bin placement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,b", [(4096, 1), (4096, 1000), (4096, 2048), (1024, 512)])
def test_a_cosine_lands_in_its_bin(n_fft, b):
    T = n_fft
    c = np.cos(2.0 * np.pi * ((b * np.arange(T)) % T) / T).astype(np.float32)[None, :]
    res = metrics.modulation_spectrum([c], n_fft)
    P = res["power"].cpu().numpy()[0, 0].astype(np.float64)
    w = bounds(c, n_fft)
    peak = float(T) if b == n_fft // 2 else T / 4.0                           # (module docstring: T at the Nyquist bin)
    assert abs(w["P"][0, b - 1] - peak) <= 1e-6 * peak                        # the checker agrees (the input is a float32 cosine)
    print("n_fft %d bin %d: peak %.6f (want %.1f, gate %.3g), largest other bin %.3g" % (n_fft, b, P[b - 1], peak, w["b_P"][0, b - 1], np.delete(P, b - 1).max()))
    assert abs(P[b - 1] - w["P"][0, b - 1]) <= w["b_P"][0, b - 1]
    assert abs(P[b - 1] - peak) <= w["b_P"][0, b - 1] + 1e-6 * peak
    assert np.delete(P, b - 1).max() < 1e-6 * T / 4.0


# ---- 3. Parseval on the kernel's own outputs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n_fft", [(24, 1024), (33, 2048), (80, 4096)])
def test_parseval_on_the_kernel_outputs(data, want, K, n_fft):
    """2 sum_{f < n/2} P_f + P_{n/2} = n var.  With w_f the weights, sum_f w_f |dP_f| <= (2 delta sum_f w_f |X_f| + n delta^2) / T and by
    Cauchy-Schwarz sum_f w_f |X_f| <= sqrt(n) sqrt(n T var): the sum of the P is within (2 delta n sqrt(T var) + n delta^2) / T of n var64,
    and the kernel's var within its own gate of var64."""
    res = metrics.modulation_spectrum(data[(K, n_fft)], n_fft)
    P, var = res["power"].cpu().numpy().astype(np.float64), res["var"].cpu().numpy().astype(np.float64)
    for i, w in enumerate(want[(K, n_fft)]):
        lhs = 2.0 * P[i][:, :-1].sum(axis=1) + P[i][:, -1]
        T, d, v64 = w["T"], w["delta"], w["var"]
        gate = (2.0 * d * n_fft * np.sqrt(T * v64) + n_fft * d * d) / T + n_fft * w["b_var"]
        err = np.abs(lhs - n_fft * var[i])
        rel = float(np.max(err / np.maximum(n_fft * v64, 1e-300))) if T > 1 else 0.0
        print("K=%d n_fft=%d T=%d: Parseval relative error %.2e, error / gate %.4f" % (K, n_fft, T, rel, float(np.max(err / np.maximum(gate, 1e-300)))))
        assert (err <= gate).all()


# ---- 4. a ragged bank equals its single calls bit for bit ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def single(data):
    out = {}
    for combo in [(K, 1024) for K in KS] + [(24, 2048), (24, 4096)]:
        res = []
        for c in data[combo]:
            r = metrics.modulation_spectrum([c], combo[1])
            res.append(tuple(r[k].cpu().numpy()[0] for k in ("power", "mean", "var")))
        out[combo] = res
    return out


@pytest.mark.parametrize("K,n_fft", [(K, 1024) for K in KS] + [(24, 2048), (24, 4096)])
def test_a_ragged_bank_equals_its_single_calls(data, single, K, n_fft):
    utts = data[(K, n_fft)]
    n = len(utts)
    for order in (list(range(n)), list(np.random.RandomState(5).permutation(n)), list(range(n))[::-1]):
        res = metrics.modulation_spectrum([utts[i] for i in order], n_fft)
        assert res["offs"].tolist() == [0] + list(np.cumsum([utts[i].shape[1] for i in order])) and res["n_fft"] == n_fft
        got = [res[k].cpu().numpy() for k in ("power", "mean", "var")]
        for pos, i in enumerate(order):
            for g, s in zip(got, single[(K, n_fft)][i]):
                assert np.array_equal(bits(g[pos]), bits(s)), (order, i)
    # a (bank, offs) pair already on the device is the same bank
    b, offs = metrics.bank(utts)
    res = metrics.modulation_spectrum((b, offs), n_fft)
    assert all(np.array_equal(bits(res["power"][i].cpu().numpy()), bits(single[(K, n_fft)][i][0])) for i in range(n))


def test_huge_neighbours_do_not_leak(data, single):
    K, n_fft = 24, 1024
    utts = data[(K, n_fft)]
    rs = np.random.RandomState(9)
    big = [(1e6 * rs.randn(K, T)).astype(np.float32) for T in (64, 65)]
    for i in (0, 1, 2, 3, 5):                                                 # T = 1, 2, 3, 63, 65 between the two
        res = metrics.modulation_spectrum([big[0], utts[i], big[1]], n_fft)
        for k, s in zip(("power", "mean", "var"), single[(K, n_fft)][i]):
            assert np.array_equal(bits(res[k][1].cpu().numpy()), bits(s)), (i, k)


# ---- 5. degenerate input ---------------------------------------------------------------------------------------------------------------------
def test_degenerate_utterances(data, single):
    K, n_fft = 24, 1024
    normal = data[(K, n_fft)][5]                                              # T = 65
    one = ck.trajectory(np.random.RandomState(1), K, 1)
    const = np.repeat((0.1 * (np.arange(K) + 1.0) * (-1.0) ** np.arange(K)).astype(np.float32)[:, None], 41, axis=1)
    silence = np.zeros((K, 64), dtype=np.float32)
    mixed = normal.copy()[:, :40]
    mixed[3] = 0.7                                                            # one constant row inside a normal utterance
    res = metrics.modulation_spectrum([normal, one, const, silence, mixed, normal], n_fft)
    P, mean, var = (res[k].cpu().numpy() for k in ("power", "mean", "var"))
    for i, c in ((1, one), (2, const), (3, silence)):
        assert (var[i] == 0.0).all() and (P[i] == 0.0).all(), i
        assert np.array_equal(mean[i], c[:, 0]), i
    assert var[4][3] == 0.0 and (P[4][3] == 0.0).all() and mean[4][3] == np.float32(0.7) and (var[4][np.arange(K) != 3] > 0).all()
    for i in (0, 5):                                                          # the neighbours are what they are alone
        for k, s in zip((P, mean, var), single[(K, n_fft)][5]):
            assert np.array_equal(bits(k[i]), bits(s))
    floor_db = 10.0 * math.log10(ck.FLOOR)
    lms = metrics.mean_log(res["power"][1:4]).cpu().numpy().astype(np.float64)
    lgv = metrics.mean_log(res["var"][1:4]).cpu().numpy().astype(np.float64)
    gate = mean_log_gate(np.full((3, 1), floor_db))[0]
    assert np.abs(lms - floor_db).max() <= gate and np.abs(lgv - floor_db).max() <= gate and abs(floor_db + 100.0) < 1e-12


# ---- 6. the two reductions, and msd end to end -------------------------------------------------------------------------------------------------
def mean_log_gate(terms64):
    """terms64 [n, R] (the float64 dB terms) -> gate [R].  A term is fl(10 fl(log10 v)): log10f is documented to 2 ulp = 4 u, the product
    one rounding; n - 1 additions in index order and the division: (4 + 1 + n) u mean|t|, one u spare.  The float32 floor differs from 1e-10
    by at most u relative: 10 log10(1 + u) = 4.35 u dB for a floored term."""
    n = terms64.shape[0]
    return ((6 + n) * U * np.abs(terms64).sum(axis=0) / n + 4.35 * U) * 1.01


def distance_gates(F, K):
    """-> relative gates (per_dim, total).  d = fl(a - b) squared: 2 u; a lane chain of ceil(F / 64) fused terms and six butterfly levels;
    the division; the square root halves what is under it and rounds once.  The total adds the chain over the rows (ceil(K / 64) + 6)."""
    per = (0.5 * (math.ceil(F / 64) + 6 + 2 + 1) + 1) * U * 1.01
    tot = (0.5 * (math.ceil(F / 64) + 6 + 2 + math.ceil(K / 64) + 6 + 1) + 1) * U * 1.01
    return per, tot


@pytest.mark.parametrize("n,R", [(1, 1), (1, 300), (5, 24 * 512), (35, 257)])
def test_mean_log_against_float64(n, R):
    rs = np.random.RandomState(n * 1000 + R)
    v = np.exp(rs.uniform(math.log(1e-9), math.log(1e4), size=(n, R))).astype(np.float32)
    v.reshape(-1)[::7] = np.float32(0.0)                                      # under the floor
    v.reshape(-1)[3::11] = np.float32(1e-12)
    got = metrics.mean_log(torch.from_numpy(v).cuda()).cpu().numpy().astype(np.float64)
    terms = 10.0 * np.log10(np.maximum(v.astype(np.float64), ck.FLOOR))
    want64 = ck.mean_log(v)
    gate = mean_log_gate(terms)
    print("mean_log n=%d R=%d: largest error / gate %.3f" % (n, R, float((np.abs(got - want64) / gate).max())))
    assert got.shape == (R,) and (np.abs(got - want64) <= gate).all()
    got3 = metrics.mean_log(torch.from_numpy(v).cuda(), floor=1e-3).cpu().numpy()
    assert np.abs(got3 - ck.mean_log(v, 1e-3)).max() <= 1e-4 and got3.min() >= -30.001


@pytest.mark.parametrize("K,n_bins,F", [(1, 1, 1), (1, 24, 24), (24, 512, 1), (24, 512, 118), (33, 1024, 1024), (80, 2048, 2047), (80, 2048, 2048)])
def test_distance_against_float64(K, n_bins, F):
    rs = np.random.RandomState(K * 10000 + n_bins + F)
    a = (-40.0 + 20.0 * rs.randn(K, n_bins)).astype(np.float32)
    b = (a + 3.0 * rs.randn(K, n_bins)).astype(np.float32)
    b[:, F:] = 1e9                                                            # bins beyond n_used must not count
    per, tot = metrics.table_distance(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), F)
    per, tot = per.cpu().numpy().astype(np.float64), float(tot.cpu()[0])
    per64, tot64 = ck.distance(a, b, F)
    g_per, g_tot = distance_gates(F, K)
    print("distance K=%d n_bins=%d F=%d: per_dim rel %.2e (gate %.2e), total rel %.2e (gate %.2e)" % (
        K, n_bins, F, float((np.abs(per - per64) / per64).max()), g_per, abs(tot - tot64) / tot64, g_tot))
    assert per.shape == (K,) and (np.abs(per - per64) <= g_per * per64).all() and abs(tot - tot64) <= g_tot * tot64
    if K == 1 and F == n_bins:                                                # a [K] table is one row of K bins: the GVD call
        per1, tot1 = metrics.table_distance(torch.from_numpy(a[0]).cuda(), torch.from_numpy(b[0]).cuda())
        assert float(per1.cpu()[0]) == float(tot1.cpu()[0]) and bits(tot1.cpu().numpy())[0] == bits(np.float32([tot]))[0]
    same_per, same_tot = metrics.table_distance(torch.from_numpy(a).cuda(), torch.from_numpy(a).cuda(), F)
    assert float(same_tot.cpu()[0]) == 0.0 and (same_per.cpu().numpy() == 0.0).all()


def mel_sets():
    """Two sets of log10-mels [80, T], 3 and 5 utterances of different lengths: a slow random walk plus white noise, the second set's
    noise term twice the first's (its modulation spectrum lies about 6 dB higher where the noise dominates)."""
    rs = np.random.RandomState(20)
    A = [(-2.0 + 0.02 * np.cumsum(rs.randn(80, T), axis=1) + 0.1 * rs.randn(80, T)).astype(np.float32) for T in (63, 80, 97)]
    B = [(-2.0 + 0.02 * np.cumsum(rs.randn(80, T), axis=1) + 0.2 * rs.randn(80, T)).astype(np.float32) for T in (64, 65, 71, 90, 101)]
    return A, B


def lms_gates(ceps, n_fft, F):
    """list of float32 cepstra -> (largest element-wise LMS gate over the first F bins, largest LGV gate): the gates of P and var pushed
    through the logarithm, |d 10 log10 v| <= (10 / ln 10) b / (v - b), averaged over the set, plus the mean-log kernel's own gate."""
    ws = [bounds(c, n_fft) for c in ceps]
    k = 10.0 / math.log(10.0)
    for w in ws:
        assert (w["b_P"][:, :F] < 0.5 * w["P"][:, :F]).all() and (w["b_var"] < 0.5 * w["var"]).all()
    g_lms = np.mean([k * w["b_P"][:, :F] / (w["P"][:, :F] - w["b_P"][:, :F]) for w in ws], axis=0)
    g_lgv = np.mean([k * w["b_var"] / (w["var"] - w["b_var"]) for w in ws], axis=0)
    g_lms = g_lms + mean_log_gate(np.stack([(10.0 * np.log10(w["P"][:, :F])).reshape(-1) for w in ws])).reshape(g_lms.shape)
    g_lgv = g_lgv + mean_log_gate(np.stack([10.0 * np.log10(w["var"]) for w in ws]))
    return float(g_lms.max()), float(g_lgv.max())


@pytest.mark.parametrize("max_hz", [None, 10.0])
def test_msd_end_to_end(max_hz):
    """The triangle inequality on the root-mean-square norm: |msd - msd64| <= max |d LMS_A| + max |d LMS_B| (a root mean square is at most
    the largest entry), plus the distance kernel's relative gate; the same for gvd.  The float64 side is the checker on the GPU's own
    cepstra.  The sets are chosen so that this gate is at most 1 % of msd64 (asserted)."""
    n_fft, n_cep = 1024, 24
    A, B = mel_sets()
    res = metrics.msd(A, B, n_cep, n_fft, max_hz)
    ca = [c.cpu().numpy() for c in metrics.split(*metrics.mel_cepstra(A, n_cep))]
    cb = [c.cpu().numpy() for c in metrics.split(*metrics.mel_cepstra(B, n_cep))]
    w = ck.msd(ca, cb, n_fft, max_hz)
    F = w["n_bins_used"]
    assert res["n_bins_used"] == F == (512 if max_hz is None else 118) and res["n_converted"] == 3 and res["n_target"] == 5 and res["n_fft"] == n_fft
    assert res["floor"] == ck.FLOOR and abs(res["max_hz"] - (ck.FRAME_RATE / 2 if max_hz is None else max_hz)) < 1e-12
    (ga, gva), (gb, gvb) = lms_gates(ca, n_fft, F), lms_gates(cb, n_fft, F)
    g_per, g_tot = distance_gates(F, n_cep)
    gate_msd = ga + gb + g_tot * w["msd"]
    gate_gvd = gva + gvb + distance_gates(n_cep, 1)[1] * w["gvd"]
    print("max_hz %s: msd %.6f dB (float64 %.6f, error %.2e, gate %.2e = %.3f %% of it); gvd %.6f dB (float64 %.6f, error %.2e, gate %.2e)" % (
        max_hz, res["msd"], w["msd"], abs(res["msd"] - w["msd"]), gate_msd, 100.0 * gate_msd / w["msd"], res["gvd"], w["gvd"], abs(res["gvd"] - w["gvd"]), gate_gvd))
    assert gate_msd <= 0.01 * w["msd"] and gate_gvd <= 0.01 * w["gvd"]
    assert abs(res["msd"] - w["msd"]) <= gate_msd and abs(res["gvd"] - w["gvd"]) <= gate_gvd
    assert (np.abs(res["msd_per_dim"].astype(np.float64) - w["msd_per_dim"]) <= ga + gb + g_per * w["msd_per_dim"]).all()
    assert np.abs(res["lms_converted"][:, :F] - w["lms_a"][:, :F]).max() <= ga and np.abs(res["lms_target"][:, :F] - w["lms_b"][:, :F]).max() <= gb
    assert np.abs(res["lgv_converted"] - w["lgv_a"]).max() <= gva and np.abs(res["lgv_target"] - w["lgv_b"]).max() <= gvb
    assert res["lms_converted"].shape == (n_cep, n_fft // 2) and res["lgv_target"].shape == (n_cep,)
    same = metrics.msd(A, A, n_cep, n_fft, max_hz)
    assert same["msd"] == 0.0 and same["gvd"] == 0.0 and (same["msd_per_dim"] == 0.0).all()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    K = 4
    rs = np.random.RandomState(2)
    long = ck.trajectory(rs, K, 1025)
    with pytest.raises(ValueError, match="utterance 1 has 1025 frames, more than n_fft = 1024"):
        metrics.modulation_spectrum([long[:, :100], long], 1024)
    assert metrics.modulation_spectrum([long], 2048)["power"].shape == (1, K, 1024)
    with pytest.raises(ValueError, match="n_fft"):
        metrics.modulation_spectrum([long[:, :100]], 512)
    with pytest.raises(ValueError, match="HIP device"):
        metrics.modulation_spectrum((torch.from_numpy(long), np.array([0, 1025])), 2048)
    bad = long[:, :100].copy()
    bad[2, 17] = np.inf
    with pytest.raises(ValueError, match="finite"):
        metrics.modulation_spectrum([bad], 1024)
    bad[2, 17] = np.nan
    with pytest.raises(ValueError, match="finite"):
        metrics.modulation_spectrum([long[:, :10], bad], 1024)
    mels = [np.zeros((80, 1025), dtype=np.float32)]
    with pytest.raises(ValueError, match="more than n_fft"):
        metrics.msd(mels, mels, 24, 1024)
    for hz in (0.0, 50.0):
        with pytest.raises(ValueError, match="max_hz"):
            metrics.msd(mels, mels, 24, 2048, hz)
    # the C ABI: poisoned outputs stay what they were
    L = _hip.lib()
    b, offs = metrics.bank([long[:, :100], long])
    table = _hip.device_constant(("metrics.ms_table", 1024), b.device, lambda: metrics.host_ms_table(1024))
    offs_d = torch.from_numpy(offs).cuda()
    outs = [torch.full((n,), 123.25, dtype=torch.float32, device="cuda") for n in (2 * K * 512, 2 * K, 2 * K)]
    calls = [(K, offs, 1024), (0, offs, 1024), (81, offs, 1024), (K, offs, 1000), (K, np.array([0, 100, 1124], dtype=np.int32), 1024),
             (K, np.array([0, 1125, 100], dtype=np.int32), 2048)]
    for K_, offs_, n_fft_ in calls:
        rc = L.mcvc_ms_power(_hip.ptr(b), b.shape[1], K_, _hip.ptr(offs_d), 2, offs_.ctypes.data, n_fft_, _hip.ptr(table), _hip.ptr(outs[0]),
                             _hip.ptr(outs[1]), _hip.ptr(outs[2]), _hip.stream())
        assert rc == MCVC_ERR_INVALID, (K_, offs_, n_fft_)
    assert L.mcvc_ms_mean_log(_hip.ptr(outs[0]), 0, 8, 1e-10, _hip.ptr(outs[1]), _hip.stream()) == MCVC_ERR_INVALID
    assert L.mcvc_ms_mean_log(_hip.ptr(outs[0]), 2, 8, 0.0, _hip.ptr(outs[1]), _hip.stream()) == MCVC_ERR_INVALID
    assert L.mcvc_ms_distance(_hip.ptr(outs[0]), _hip.ptr(outs[0]), 2, 4, 5, _hip.ptr(outs[1]), _hip.ptr(outs[2]), _hip.stream()) == MCVC_ERR_INVALID
    torch.cuda.synchronize()
    assert all(bool((o == 123.25).all()) for o in outs)


# ---- 8. the command line -------------------------------------------------------------------------------------------------------------------------
def seeded_mels(seed, lengths):
    rs = np.random.RandomState(seed)
    return [(-2.0 + np.cumsum(0.1 * rs.randn(80, T), axis=1) + 0.2 * rs.randn(80, T)).astype(np.float32) for T in lengths]


def test_cli_msd_without_parallel_sentences(tmp_path, capsys, golden_dir):
    from data_preprocessing.audio2mel import Audio2Mel
    conv = seeded_mels(4, (70, 131, 64))
    cdir = tmp_path / "run" / "exp" / "converted_mel"
    os.makedirs(str(cdir))
    for i, m in zip((0, 1, 5), conv):                                         # index 5 lies beyond the two references
        np.save(str(cdir / ("%d-converted_SRC_to_TGT.npy" % i)), m)
    wav_dir = os.path.join(golden_dir, "audio")
    base = ["--save_dir", str(tmp_path / "run"), "--name", "exp", "--target_wav_dir", wav_dir]
    rep = evaluate.main(base + ["--msd", "--no_mcd", "--msd_n_fft", "1024"])
    line = capsys.readouterr().out
    disk = json.load(open(str(tmp_path / "run" / "exp" / "metrics.json")))
    assert disk == json.loads(json.dumps(rep))
    refs = Audio2Mel().bank(evaluate.wav_dir_waves(wav_dir))
    want = metrics.msd(conv, refs, 24, 1024)
    half = metrics.msd(refs[0::2], refs[1::2], 24, 1024)
    m = disk["msd"]
    assert m["msd"] == want["msd"] and m["gvd"] == want["gvd"] and m["target_split_half_msd"] == half["msd"] and m["msd"] > 0.0
    assert m["msd_per_dim"] == [float(v) for v in want["msd_per_dim"]] and m["lgv_converted"] == [float(v) for v in want["lgv_converted"]]
    assert m["lgv_target"] == [float(v) for v in want["lgv_target"]]
    assert (m["n_converted"], m["n_target"], m["n_fft"], m["floor"]) == (3, 2, 1024, 1e-10) and abs(m["max_hz"] - 22050.0 / 512.0) < 1e-9
    assert "not WORLD" in m["unit"] and "baseline_msd" not in m
    assert set(disk) == {"n_cep", "n_utterances", "utterances", "msd"} and disk["n_utterances"] == 3
    assert [(u["index"], u["frames_converted"]) for u in disk["utterances"]] == [(0, 70), (1, 131), (5, 64)]
    assert all(set(u) == {"index", "file", "frames_converted"} for u in disk["utterances"])
    assert "MSD %.3f dB, GVD %.3f dB" % (want["msd"], want["gvd"]) in line and "target split-half MSD" in line and "MCD" not in line
    # without --no_mcd the index contract holds as before
    with pytest.raises(ValueError, match="converted utterance 5 has no reference"):
        evaluate.main(base + ["--msd", "--msd_n_fft", "1024"])
    # a band limit reaches the kernel
    lim = evaluate.main(base + ["--msd", "--no_mcd", "--msd_n_fft", "1024", "--msd_max_hz", "10"])
    assert lim["msd"]["msd"] == metrics.msd(conv, refs, 24, 1024, 10.0)["msd"] and lim["msd"]["max_hz"] == 10.0
    # a single target utterance has no split half
    one = tmp_path / "one"
    os.makedirs(str(one))
    import shutil
    shutil.copy(os.path.join(wav_dir, "real_VCC2SF3.wav"), str(one / "a.wav"))
    rep1 = evaluate.main(["--save_dir", str(tmp_path / "run"), "--name", "exp", "--target_wav_dir", str(one), "--msd", "--no_mcd"])
    assert rep1["msd"]["target_split_half_msd"] is None and rep1["msd"]["n_target"] == 1 and rep1["msd"]["n_fft"] == 4096


def write_speaker(root, spk, mels):
    import pickle
    allf = np.concatenate(mels, axis=1)
    mean, std = allf.mean(axis=1, keepdims=True), allf.std(axis=1, keepdims=True)
    os.makedirs(os.path.join(root, spk), exist_ok=True)
    with open(os.path.join(root, spk, "%s_normalized.pickle" % spk), "wb") as fh:
        pickle.dump([((m - mean) / std).astype(np.float32) for m in mels], fh)
    np.savez(os.path.join(root, spk, "%s_norm_stat.npz" % spk), mean=mean, std=std)


def test_cli_msd_beside_mcd_changes_nothing_else(tmp_path, capsys):
    conv, tgt, src = seeded_mels(5, (70, 131, 64)), seeded_mels(6, (83, 120, 65, 90)), seeded_mels(7, (70, 131, 64))
    cache = str(tmp_path / "cache")
    write_speaker(cache, "TGT", tgt)
    write_speaker(cache, "SRC", src)
    cdir = tmp_path / "run" / "exp" / "converted_mel"
    os.makedirs(str(cdir))
    for i, m in enumerate(conv):
        np.save(str(cdir / ("%d-converted_SRC_to_TGT.npy" % i)), m)
    base = ["--save_dir", str(tmp_path / "run"), "--name", "exp", "--preprocessed_data_dir", cache, "--target_speaker_id", "TGT", "--source_speaker_id", "SRC"]
    plain = evaluate.main(base)
    line_plain = capsys.readouterr().out.strip()
    with_msd = evaluate.main(base + ["--msd", "--msd_n_fft", "2048"])
    line_msd = capsys.readouterr().out.strip()
    assert "msd" not in plain and "msd" in with_msd
    assert {k: v for k, v in with_msd.items() if k != "msd"} == plain
    refs, srcs = evaluate.speaker_mels(cache, "TGT"), evaluate.speaker_mels(cache, "SRC")
    m = with_msd["msd"]
    assert m["n_target"] == 4 and m["n_converted"] == 3                       # all four target utterances, not the three index-matched ones
    assert m["msd"] == metrics.msd(conv, refs, 24, 2048)["msd"]
    b = metrics.msd(srcs, refs, 24, 2048)
    assert m["baseline_msd"] == b["msd"] and m["baseline_gvd"] == b["gvd"]
    head, tail = line_plain.rsplit(" -> ", 1)
    assert line_msd.startswith(head + " | MSD ") and line_msd.endswith(" -> " + tail) and "unconverted baseline MSD" in line_msd
