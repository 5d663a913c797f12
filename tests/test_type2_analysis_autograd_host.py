"""CPU tests of the float64 model of the type-2 analysis chain (tests/type2_analysis_autograd_model.py): its forward
against the restatement of the reference that the golden tests use (tests/type2_model.py + tests/true_envelope_model.py),
its gradient against a central difference along a random direction with the decisions held, and that the plans refuse
more than 64 coefficient columns before any device work."""
import numpy as np
import pytest
import torch

import compressed_analysis_autograd_model as cmodel
import true_envelope_model as tem
import type2_analysis_autograd_model as t2m
import type2_model

FS, N = 16000, 1024


def _utts():
    rng = np.random.RandomState(5)
    out = []
    for n_voiced, n_unvoiced, gap in ((12, 6, True), (7, 3, False)):
        sig, pm_sec, voi = t2m.utterance(rng, FS, N, n_voiced, n_unvoiced, gap=gap)
        out.append((sig, FS, pm_sec, voi))
    return out


def test_chain_model_equals_the_reference_restatement():
    utts = _utts()
    tab = t2m.batch_tables(utts)
    sig = torch.from_numpy(np.concatenate([u[0] for u in utts]).astype(np.float64))
    assert np.max(tab["left2"] + tab["right2"] + 1) > N          # a two-period frame that the transform truncates
    refs = [type2_model.analysis(u[0], FS, u[2], u[3], N) for u in utts]
    mag2 = np.concatenate([r["mag2"] for r in refs])
    env_ref, iters = tem.true_envelope(mag2, "abs", 600, 0.1)
    rows = t2m.out_rows(tab)
    it_all = np.ones(tab["pos"].size, dtype=np.int32)
    it_all[rows] = iters
    env, real, imag, _used, _margin = t2m.forward_torch(sig, tab, N, it_all)
    for got, ref in ((env.numpy()[rows], env_ref), (real.numpy()[rows], np.concatenate([r["real"] for r in refs])),
                     (imag.numpy()[rows], np.concatenate([r["imag"] for r in refs]))):
        assert np.max(np.abs(got - ref)) <= 1e-9 * np.max(np.abs(ref))
    for u, r in enumerate(refs):                                 # the two-period table is the even / odd subsets' one
        a, b = tab["frame_off"][u], tab["frame_off"][u + 1]
        assert np.array_equal(tab["left2"][a:b], r["left2"]) and np.array_equal(tab["right2"][a:b], r["right2"])


@pytest.mark.parametrize("norm", [False, True])
def test_chain_model_gradient_against_a_central_difference(norm):
    utts = _utts()[1:]
    tab = t2m.batch_tables(utts)
    sig = utts[0][0].astype(np.float64)
    F = tab["pos"].size
    iters = np.full(F, 6, dtype=np.int32)
    wm, wp = cmodel.warps(N, FS, 60, 45)
    rows = t2m.out_rows(tab)
    rows_tab = {"row0": rows, "row1": rows, "rowt": np.zeros(rows.size), "voi": np.arange(rows.size) % 3 != 0}
    _e, _r, _i, used, _m = t2m.forward_torch(torch.from_numpy(sig), tab, N, iters)
    fn = lambda x: t2m.compressed_torch(x, tab, rows_tab, N, iters, used, wm, wp, b_norm_mag=norm)[:3]   # noqa: E731
    rng = np.random.RandomState(1)
    grads = [rng.randn(rows.size, 60), rng.randn(rows.size, 45), rng.randn(rows.size, 45)]
    pre = fn(torch.from_numpy(sig))
    for k in (1, 2):                                             # keep clear of the clip's corner
        grads[k][np.abs(np.abs(pre[k].numpy()) - 1.0) < 1e-3] = 0.0
    g = t2m.grads_of(sig, fn, grads)
    d = rng.randn(sig.size)
    step = 1e-6
    val = lambda x: float(sum((o.numpy() * w).sum() for o, w in zip(fn(torch.from_numpy(x)), grads)))   # noqa: E731
    fd = (val(sig + step * d) - val(sig - step * d)) / (2 * step)
    assert abs(fd - float(g @ d)) <= 1e-5 * max(abs(fd), 1.0)


def test_more_than_64_columns_are_refused_by_name():
    from magphase_amd.plans import Type2CompressedAnalysisPlan

    for name, kw in (("mag_dim", {"mag_dim": 65, "phase_dim": 45}), ("phase_dim", {"mag_dim": 60, "phase_dim": 65})):
        plan = Type2CompressedAnalysisPlan.__new__(Type2CompressedAnalysisPlan)
        plan.mag_dim, plan.phase_dim = kw["mag_dim"], kw["phase_dim"]
        with pytest.raises(NotImplementedError, match=name):
            plan.check_differentiable()


def test_chain_model_against_the_golden_file(golden_dir):
    """The chain model's forward on the golden utterances (tests/golden/g16_type2.npz: phase rows, envelope in dB and pass
    counts of the reference), within the bounds tests/test_type2_host.py holds tests/type2_model.py to."""
    from magphase_amd import hostmath as hm
    from magphase_amd import synthetic as syn

    g = np.load(golden_dir + "/g16_type2.npz")
    for tag in g["tags"]:
        tag = str(tag)
        v_sig, fs = syn.pcm_to_float(g[tag + "_pcm"]), int(g[tag + "_fs"])
        n_fft, step = hm.define_fft_len(fs), int(g[tag + "_step"])
        tab = t2m.batch_tables([(v_sig, fs, g[tag + "_pm_sec"], g[tag + "_voi"])])
        rows = t2m.out_rows(tab)
        iters = np.ones(tab["pos"].size, dtype=np.int32)
        iters[rows] = g[tag + "_passes"]
        with torch.no_grad(), np.errstate(divide="ignore", invalid="ignore"):
            env, real, imag, _u, _m = t2m.forward_torch(torch.from_numpy(v_sig.astype(np.float64)), tab, n_fft, iters)
            db = 20.0 * np.log10(env.numpy()[rows][:, ::step])
        np.testing.assert_allclose(real.numpy()[rows][:, ::step], g[tag + "_real"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(imag.numpy()[rows][:, ::step], g[tag + "_imag"], rtol=0, atol=1e-6)
        ref = g[tag + "_env_db"].astype(np.float64)
        assert np.array_equal(np.isnan(db), np.isnan(ref))
        ok = ~np.isnan(ref)
        assert np.max(np.abs(db[ok] - ref[ok])) < 1e-4
