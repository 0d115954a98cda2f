"""GPU checks of the objective-evaluation kernels (csrc/dtw_kernels.hip through mask_cyclegan_vc/metrics.py and the evaluate CLI) against
the float64 restatement tests/dtw_checker.py.

Shapes: the smallest at which a sweep in strips of 64 rows can go wrong -- single cells and single rows / columns, one row short of a
strip, a full strip, one row into the second strip, columns beyond two strips, three strips against a ragged width -- at K = 1 (all but
one feature row padded), 24 (the metric's default, a whole number of eight-row groups) and 80 (the limit).

The cost gate |cost - cost64| <= (Tx + Ty + K + 8) 2^-23 cost64 is derived, not measured: each d carries at most about K / 2 + 4
roundings (K fused terms under a square root, the root, the scale), a path sums at most Tx + Ty positive terms one after the other, the
minimum over paths inherits the bound of every path, and a factor 2 of margin is included.  For float data paths are never compared with
the checker's (a tie within rounding may legitimately go the other way); they are checked for validity and for their own float64 cost."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dtw_checker as ck  # noqa: E402
from mask_cyclegan_vc import _hip, evaluate, metrics  # noqa: E402

SHAPES = [(1, 1), (1, 5), (5, 1), (2, 3), (63, 64), (64, 64), (65, 64), (64, 129), (130, 67), (200, 37)]
KS = (1, 24, 80)
SCALE = 1.7
U = 2.0 ** -23


def bound(Tx, Ty, K):
    return (Tx + Ty + K + 8) * U


def make(K, seed=0):
    rs = np.random.RandomState(1000 * K + seed)
    xs = [rs.randn(K, Tx).astype(np.float32) for Tx, _ in SHAPES]
    ys = [(rs.randn(K, Ty) + 0.25).astype(np.float32) for _, Ty in SHAPES]
    return xs, ys


@pytest.fixture(scope="module")
def data():
    return {K: make(K) for K in KS}


@pytest.fixture(scope="module")
def want(data):
    """float64 results on the same float32 features, computed once: K -> [(cost, length, path)]."""
    return {K: [ck.dtw(x, y, SCALE) for x, y in zip(*data[K])] for K in KS}


@pytest.fixture(scope="module")
def single(data):
    """Every pair as a call of its own, with paths: K -> [(cost float32 scalar, length, path numpy)]."""
    out = {}
    for K in KS:
        res = []
        for x, y in zip(*data[K]):
            c, n, p = metrics.dtw([x], [y], SCALE, return_path=True)
            res.append((c.cpu().numpy()[0], int(n.cpu().numpy()[0]), p[0].cpu().numpy()))
        out[K] = res
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("K", KS)
def test_cost_against_float64(single, want, K):
    for (Tx, Ty), (c, n, _), (c64, n64, _) in zip(SHAPES, single[K], want[K]):
        rel = abs(float(c) - c64) / c64
        print("K=%d %dx%d: cost %.9g (float64 %.12g), relative error %.2e, bound %.2e; length %d (float64 %d)" % (K, Tx, Ty, c, c64, rel, bound(Tx, Ty, K), n, n64))
        assert np.isfinite(c) and rel <= bound(Tx, Ty, K)
        assert max(Tx, Ty) <= n <= Tx + Ty - 1


@pytest.mark.parametrize("K", KS)
def test_paths_are_valid_and_as_cheap_as_the_optimum(data, single, want, K):
    for (Tx, Ty), x, y, (c, n, p), (c64, _, _) in zip(SHAPES, data[K][0], data[K][1], single[K], want[K]):
        assert p.dtype == np.int32 and p.shape == (n, 2)                    # length from the recurrence = rows the backtrack wrote
        assert ck.path_is_valid(p, Tx, Ty), (Tx, Ty)
        own = ck.path_cost(x, y, p, SCALE)
        rel = abs(own - c64) / c64
        print("K=%d %dx%d: float64 cost along the returned path %.12g, optimum %.12g, relative %.2e, bound %.2e" % (K, Tx, Ty, own, c64, rel, bound(Tx, Ty, K)))
        assert own >= c64 * (1.0 - 1e-15) and rel <= bound(Tx, Ty, K)


@pytest.mark.parametrize("shape", [(70, 90), (64, 64)])
def test_integer_features_pin_the_tie_rule(shape):
    """Integer features in [-3, 3], K = 1, scale = 1: every quantity is exact in float32 and ties abound, so cost, length and the whole path
    equal the checker's -- in both orders of the banks."""
    Tx, Ty = shape
    rs = np.random.RandomState(Tx * 1000 + Ty)
    x = rs.randint(-3, 4, size=(1, Tx)).astype(np.float32)
    y = rs.randint(-3, 4, size=(1, Ty)).astype(np.float32)
    for a, b in ((x, y), (y, x)):
        c64, n64, p64 = ck.dtw(a, b)
        c, n, p = metrics.dtw([a], [b], 1.0, return_path=True)
        print("integer case %dx%d: cost %g length %d (checker %g, %d)" % (a.shape[1], b.shape[1], float(c[0]), int(n[0]), c64, n64))
        assert float(c[0]) == c64 and int(n[0]) == n64
        assert np.array_equal(p[0].cpu().numpy(), p64)
    assert float(metrics.dtw([x], [y])[0][0]) == float(metrics.dtw([y], [x])[0][0])


@pytest.mark.parametrize("K", (1, 24))
def test_identities_across_a_strip_boundary(K):
    T = 65
    x = np.random.RandomState(7 + K).randn(K, T).astype(np.float32)
    c, n, p = metrics.dtw([x], [x], SCALE, return_path=True)
    assert float(c[0]) == 0.0 and int(n[0]) == T
    assert np.array_equal(p[0].cpu().numpy(), np.stack([np.arange(T)] * 2, axis=1))
    x2 = np.repeat(x, 2, axis=1)
    for a, b in ((x, x2), (x2, x)):
        c, n, p = metrics.dtw([a], [b], SCALE, return_path=True)
        assert float(c[0]) == 0.0 and int(n[0]) == 2 * T
        assert ck.path_is_valid(p[0].cpu().numpy(), a.shape[1], b.shape[1])


@pytest.mark.parametrize("K", KS)
def test_ragged_batch_equals_its_single_calls(data, single, K):
    xs, ys = data[K]
    order = np.random.RandomState(5).permutation(len(SHAPES))
    c, n, p = metrics.dtw([xs[i] for i in order], [ys[i] for i in order], SCALE, return_path=True)
    c, n = c.cpu().numpy(), n.cpu().numpy()
    for k, i in enumerate(order):
        assert bits(c[k:k + 1])[0] == bits(np.array([single[K][i][0]]))[0] and n[k] == single[K][i][1], SHAPES[i]
        assert np.array_equal(p[k].cpu().numpy(), single[K][i][2]), SHAPES[i]
    # the two banks swapped: again the batch is its single calls, and the cost is symmetric within the bound
    cs, ns, ps = metrics.dtw([ys[i] for i in order], [xs[i] for i in order], SCALE, return_path=True)
    cs, ns = cs.cpu().numpy(), ns.cpu().numpy()
    for k, i in enumerate(order):
        Tx, Ty = SHAPES[i]
        c1, n1, p1 = metrics.dtw([ys[i]], [xs[i]], SCALE, return_path=True)
        assert bits(cs[k:k + 1])[0] == bits(c1.cpu().numpy())[0] and ns[k] == int(n1[0])
        assert np.array_equal(ps[k].cpu().numpy(), p1[0].cpu().numpy())
        assert ck.path_is_valid(p1[0].cpu().numpy(), Ty, Tx)
        assert abs(float(cs[k]) - float(c[k])) <= 2.0 * bound(Tx, Ty, K) * float(c[k])


@pytest.mark.parametrize("K", KS)
def test_default_call_needs_no_matrix(data, single, K):
    xs, ys = data[K]
    c, n = metrics.dtw(xs, ys, SCALE)
    c, n = c.cpu().numpy(), n.cpu().numpy()
    for i in range(len(SHAPES)):
        assert bits(c[i:i + 1])[0] == bits(np.array([single[K][i][0]]))[0] and n[i] == single[K][i][1]
    xo = np.concatenate([[0], np.cumsum([t[0] for t in SHAPES])])
    yo = np.concatenate([[0], np.cumsum([t[1] for t in SHAPES])])
    assert metrics.plan(xo, yo, False)[1] == 0                                # not one byte of workspace
    assert metrics.plan(xo, yo, True)[1] >= sum(a * b for a, b in SHAPES)
    assert _hip.lib().mcvc_dtw_launches(0) == 1


def raw_run(xs, ys, want_path, fill):
    """The C ABI with buffers of this test's own: outputs and workspace pre-filled with ``fill`` (bytes)."""
    L = _hip.lib()
    xb, xo = metrics.bank(xs)
    yb, yo = metrics.bank(ys)
    table, ws_bytes, rows = metrics.plan(xo, yo, want_path)
    n = table.shape[0]
    td = torch.from_numpy(table).cuda()
    cost = torch.full((n * 4,), fill, dtype=torch.uint8, device="cuda")
    length = torch.full((n * 4,), fill, dtype=torch.uint8, device="cuda")
    ws = torch.full((max(ws_bytes, 16),), fill, dtype=torch.uint8, device="cuda")
    path = torch.full((max(rows, 1) * 8,), fill, dtype=torch.uint8, device="cuda") if want_path else None
    rc = L.mcvc_dtw_run(_hip.ptr(xb), xb.shape[1], _hip.ptr(yb), yb.shape[1], xb.shape[0], SCALE, xo.ctypes.data, yo.ctypes.data, _hip.ptr(td), n,
                        _hip.ptr(cost), _hip.ptr(length), _hip.ptr(path), _hip.ptr(ws), ws_bytes, _hip.stream())
    assert rc == 0
    torch.cuda.synchronize()
    lens = length.view(torch.int32).cpu().numpy()
    paths = None
    if want_path:
        pr = path.view(torch.int32).view(-1, 2).cpu().numpy()
        paths = [pr[int(table[p, 5]):int(table[p, 5]) + int(lens[p])] for p in range(n)]
    return cost.view(torch.float32).cpu().numpy(), lens, paths


@pytest.mark.parametrize("K", (24, 80))
def test_streams_and_uninitialised_memory(data, single, K):
    xs, ys = data[K]
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        c, n, p = metrics.dtw(xs, ys, SCALE, return_path=True)
        c, n, p = c.cpu().numpy(), n.cpu().numpy(), [q.cpu().numpy() for q in p]
    torch.cuda.current_stream().wait_stream(st)
    for fill in (0xFF, 0x00):                                                 # 0xFF: float NaN, length / path -1, unknown direction bytes
        cr, nr, pr = raw_run(xs, ys, True, fill)
        c0, n0, _ = raw_run(xs, ys, False, fill)
        for i in range(len(SHAPES)):
            for cc, nn in ((c, n), (cr, nr), (c0, n0)):
                assert bits(cc[i:i + 1])[0] == bits(np.array([single[K][i][0]]))[0] and nn[i] == single[K][i][1], (SHAPES[i], fill)
            assert np.array_equal(p[i], single[K][i][2]) and np.array_equal(pr[i], single[K][i][2]), (SHAPES[i], fill)


def test_cepstra_against_float64():
    rs = np.random.RandomState(11)
    Ts = (1, 2, 63, 65)
    mels = [(-2.0 + 1.5 * rs.randn(80, T)).astype(np.float32) for T in Ts]
    for n_cep in (1, 24, 79):
        out, offs = metrics.mel_cepstra(mels, n_cep)
        assert tuple(out.shape) == (n_cep, sum(Ts)) and out.dtype == torch.float32 and offs.tolist() == [0, 1, 3, 66, 131]
        B = ck.dct_basis(n_cep)
        worst = 0.0
        for mel, c in zip(mels, metrics.split(out, offs)):
            m64 = np.log(10.0) * mel.astype(np.float64)
            gate = (80 + 8) * U * (np.abs(B) @ np.abs(m64))
            err = np.abs(c.cpu().numpy().astype(np.float64) - B @ m64)
            worst = max(worst, float((err / gate).max()))
            assert (err <= gate).all()
        print("n_cep %d: largest error / gate %.3f" % (n_cep, worst))
    single_out, _ = metrics.mel_cepstra([mels[2]], 24)                      # a bank equals its single calls
    assert torch.equal(single_out, metrics.mel_cepstra(mels, 24)[0][:, 3:66])


def synthetic_pairs(seed=3):
    """Three (converted, target) log-mel pairs: smooth spectra, the target a time-warped, perturbed copy."""
    rs = np.random.RandomState(seed)
    conv, tgt = [], []
    for Tx, Ty in ((70, 83), (130, 120), (64, 65)):
        base = -2.0 + np.cumsum(0.15 * rs.randn(80, Tx), axis=1) + 0.5 * np.sin(np.arange(80) / 7.0)[:, None]
        pos = np.clip(np.round(np.linspace(0, Tx - 1, Ty) + rs.uniform(-1.5, 1.5, Ty)).astype(int), 0, Tx - 1)
        conv.append(base.astype(np.float32))
        tgt.append((base[:, pos] + 0.1 * rs.randn(80, Ty)).astype(np.float32))
    return conv, tgt


def test_mcd_end_to_end():
    conv, tgt = synthetic_pairs()
    res = metrics.mcd(conv, tgt, 24)
    cx, xo = metrics.mel_cepstra(conv, 24)
    cy, yo = metrics.mel_cepstra(tgt, 24)
    assert res["n_cep"] == 24 and res["frames_converted"].tolist() == [70, 130, 64] and res["frames_target"].tolist() == [83, 120, 65]
    for k, (a, b) in enumerate(zip(metrics.split(cx, xo), metrics.split(cy, yo))):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        c64, n64, _ = ck.dtw(a, b, ck.MCD_SCALE)                              # the checker on the GPU's own cepstra
        got = res["mcd"][k] * res["length"][k]
        rel = abs(got - c64) / c64
        print("pair %d: MCD %.4f dB over %d path frames (checker %.4f over %d), cost relative error %.2e" % (k, res["mcd"][k], res["length"][k], c64 / n64, n64, rel))
        assert rel <= bound(a.shape[1], b.shape[1], 24)
        assert res["length"][k] == n64 and abs(res["mcd"][k] - c64 / n64) <= bound(a.shape[1], b.shape[1], 24) * c64 / n64
    assert abs(res["mean"] - res["mcd"].mean()) <= 1e-12
    assert 0.0 < res["mean"] < 50.0


def write_speaker(root, spk, mels):
    """A preprocessed cache as the trainer reads it: standardised utterances + norm_stat."""
    allf = np.concatenate(mels, axis=1)
    mean, std = allf.mean(axis=1, keepdims=True), allf.std(axis=1, keepdims=True)
    os.makedirs(os.path.join(root, spk), exist_ok=True)
    with open(os.path.join(root, spk, "%s_normalized.pickle" % spk), "wb") as fh:
        pickle.dump([((m - mean) / std).astype(np.float32) for m in mels], fh)
    np.savez(os.path.join(root, spk, "%s_norm_stat.npz" % spk), mean=mean, std=std)


def test_evaluate_cli(tmp_path, capsys):
    conv, tgt = synthetic_pairs()
    src = [(m + 0.4 * np.linspace(-1.0, 1.0, 80, dtype=np.float32)[:, None] ** 2).astype(np.float32) for m in conv]      # another spectral tilt
    cache = str(tmp_path / "cache")
    write_speaker(cache, "TGT", tgt)
    write_speaker(cache, "SRC", src)
    cdir = tmp_path / "run" / "exp" / "converted_mel"
    os.makedirs(str(cdir))
    for i, m in enumerate(conv):
        np.save(str(cdir / ("%d-converted_SRC_to_TGT.npy" % i)), m)
    base = ["--save_dir", str(tmp_path / "run"), "--name", "exp", "--preprocessed_data_dir", cache, "--target_speaker_id", "TGT"]
    rep = evaluate.main(base)
    assert "MCD over 3 utterances" in capsys.readouterr().out
    disk = json.load(open(str(tmp_path / "run" / "exp" / "metrics.json")))
    assert disk == json.loads(json.dumps(rep)) and "baseline" not in disk
    refs = evaluate.speaker_mels(cache, "TGT")                                 # what the CLI compared against: the de-normalised cache
    want = metrics.mcd(conv, refs, 24)
    assert disk["n_cep"] == 24 and disk["n_utterances"] == 3
    for k, u in enumerate(disk["utterances"]):
        assert u["index"] == k and u["mcd"] == float(want["mcd"][k]) and u["length"] == int(want["length"][k])
        assert u["frames_converted"] == conv[k].shape[1] and u["frames_target"] == tgt[k].shape[1]
    assert disk["mean"] == float(want["mcd"].mean()) and disk["std"] == float(want["mcd"].std()) and disk["median"] == float(np.median(want["mcd"]))
    # the unconverted baseline
    disk = evaluate.main(base + ["--source_speaker_id", "SRC", "--n_cep", "13"])
    b = metrics.mcd(evaluate.speaker_mels(cache, "SRC"), refs, 13)
    assert disk["n_cep"] == 13 and disk["baseline"]["mean"] == float(b["mcd"].mean())
    assert [u["baseline_mcd"] for u in disk["utterances"]] == [float(v) for v in b["mcd"]]
    assert all(u["frames_source"] == conv[k].shape[1] for k, u in enumerate(disk["utterances"]))
    # an index without a reference
    np.save(str(cdir / "7-converted_SRC_to_TGT.npy"), conv[0])
    with pytest.raises(ValueError, match="converted utterance 7 has no reference"):
        evaluate.main(base)
