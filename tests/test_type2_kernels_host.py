"""
CPU: the references of the type-2 kernel tests (tests/type2_kernels_model.py) against the models the rest of the suite
already trusts -- tests/type2_model.py and the reference's gains on the rows of g16_type2.npz, tests/type2_synthesis_model.py
and the reference's rms_noise on the cases of g17_type2_synthesis.npz -- and the transform-free identity against the
rfft form on every frame shape the GPU tests launch.  These checks guard the reference; the kernels are compared with
it in tests/test_gpu_type2_kernels.py only.
"""
import numpy as np
import pytest

import type2_kernels_model as t2k
import type2_model as t2m
import type2_synthesis_model as t2s
from magphase_amd import hostmath as hm
from magphase_amd import synthetic as syn
from oracle import magphase_oracle as orc


def test_frame_gain_ref_equals_the_analysis_model_and_the_golden_gains(golden_dir):
    g = np.load(golden_dir + "/g16_type2.npz")
    n_voi = n_unv = 0
    for tag in (str(t) for t in g["tags"]):
        x, fs = syn.pcm_to_float(g[tag + "_pcm"]).astype(np.float64), int(g[tag + "_fs"])
        N = hm.define_fft_len(fs)
        pm_sec, voi = hm.clean_epochs(g[tag + "_pm_sec"], g[tag + "_voi"], check_len_smpls=x.size, fs=fs)
        pm, left, right = hm.frame_bounds(pm_sec * fs, x.size)
        ref = np.array([t2k.frame_gain_ref(x, int(p), int(a), int(b), v == 1, N) for p, a, b, v in zip(pm, left, right, voi)])
        model = np.array([t2m.gain(x, int(p), int(a), int(b), v == 1, N) for p, a, b, v in zip(pm, left, right, voi)])
        assert ref.dtype == np.longdouble
        n_voi, n_unv = n_voi + int(np.sum(voi == 1)), n_unv + int(np.sum(voi != 1))
        # the same arithmetic in float64 and in longdouble: one product per sample (voiced), two sums of n terms (unvoiced)
        n = (left + right + 1).astype(np.float64)
        tol = np.where(voi == 1, 2.0, 2.0 * n) * t2k.EPS
        assert np.all(np.abs(ref.astype(np.float64) - model) <= tol * np.abs(model))
        gold = g[tag + "_gain"]
        assert gold.shape == ref[1:].shape
        assert np.all(np.abs(ref[1:].astype(np.float64) - gold) <= tol[1:] * np.abs(gold))
        # the model's count of over-long frames is the number of warnings the reference raised
        assert t2m.analysis(x, fs, g[tag + "_pm_sec"], g[tag + "_voi"], N)["n_warn"] == int(g[tag + "_n_warn"])
    assert n_voi >= 10 and n_unv >= 10


def test_noise_refs_equal_the_synthesis_model_and_the_golden_rms():
    g17, g16 = t2s.golden()
    for i in range(t2s.n_cases(g17)):
        name, feats, fs, kw, seed = t2s.case_inputs(g17, g16, i)
        N = kw["fft_len"] or hm.define_fft_len(fs)
        v_shift, v_pm, v_voi, _, ns_len = t2s.frame_tables(feats[3], fs, kw["const_rate_ms"])
        np.random.seed(seed)
        noise = np.random.uniform(-1, 1, ns_len)
        frames = t2s.noise_frames(noise, v_pm, v_voi, kw["b_voi_ap_win"])
        _, left, right, _ = orc.frame_bounds(v_pm, ns_len)
        pm = np.asarray(v_pm, dtype=np.int64)
        wt = v_voi & kw["b_voi_ap_win"]
        power = np.array([t2k.noise_power_ref(noise, int(p), int(a), int(b), bool(w), N)
                          for p, a, b, w in zip(pm, left, right, wt)])
        # frame by frame against the model's own placement and transform ...
        spec = np.fft.fft(np.fft.fftshift(orc.frm_list_to_matrix(frames, v_shift, N), axes=1))[:, :N // 2 + 1]
        want = np.sum(np.abs(spec) ** 2, axis=1)
        assert np.all(np.abs(power - want) <= 1e-13 * want), name
        for f in (0, len(frames) // 2, len(frames) - 1):
            assert np.array_equal(t2k.noise_frame(noise, int(pm[f]), int(left[f]), int(right[f]), bool(wt[f])), frames[f])
        # ... and the utterance's rms against the model's identity form and the reference's recorded rms_noise
        rms = t2k.noise_rms_ref(power, [0, power.size], N)[0]
        assert abs(rms / t2s.rms_from_frames(frames, N) - 1.0) <= 1e-13, name
        assert abs(rms / float(g17[name + "_rms"]) - 1.0) <= 1e-10, name
    off = [0, 3, 3, 5]
    r = t2k.noise_rms_ref(np.array([1.0, 2.0, 3.0, 8.0, 10.0]), off, 1024)
    assert r[0] == np.sqrt(6.0 / (3 * 513)) and np.isnan(r[1]) and r[2] == np.sqrt(18.0 / (2 * 513))


@pytest.mark.parametrize("N", t2k.FFT_LENS)
@pytest.mark.parametrize("kind", t2k.SIGNALS)
def test_identity_equals_the_rfft_form_on_every_launched_shape(N, kind):
    left, right, wtype, parity = t2k.frame_table(N, 4 * len(t2k.shapes(N)) + 40, gain=False)
    pos, n = t2k.layout(left, right, parity)
    x = t2k.make_signal(kind, n)
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    n_ext = 0
    for p, L, R, w in zip(pos, left, right, wtype):
        p, L, R = int(p), int(L), int(R)
        ext = not t2k.noise_in_domain(L, R, N)
        n_ext += ext
        if ext:
            with pytest.raises(ValueError):
                t2k.noise_power_ref(x, p, L, R, w, N)
        ref = t2k.noise_power_ref(x, p, L, R, w, N, extended=ext)
        ident = t2s.rms_from_frames([t2k.noise_frame(x, p, L, R, w)], N) ** 2 * (N // 2 + 1)
        assert abs(ident - ref) <= t2k.noise_power_bound(N) * ref, (L, R, w)
        if kind == "zeros":
            assert ref == 0.0 and ident == 0.0
    assert n_ext == 20   # (N/2 - 1, N/2), (N/2, N/2) and the three longer frames, each at two offsets and with both windows
    # in the domain, the extension (frame at index 0) and the reference's placement have the same power
    for L, R in t2k.shapes(N):
        if t2k.noise_in_domain(L, R, N):
            a = t2k.noise_power_ref(x, L, L, R, 1, N)
            b = t2k.noise_power_ref(x, L, L, R, 1, N, extended=True)
            assert abs(a - b) <= t2k.noise_power_bound(N) * a


def test_tables_hold_what_the_issue_lists():
    for N in t2k.FFT_LENS:
        s = t2k.shapes(N, gain=True)
        for want in t2k.BASE_SHAPES + [(N // 2 - 1, N // 2 - 1), (N // 2 - 1, N // 2), (N // 2, N // 2), (N - 1, 5), (N, 5),
                                       (N + 7, 40), (5, N + 7)]:
            assert want in s
        left, right, flag, parity = t2k.frame_table(N, 2061, gain=True)
        assert left.size == 2061 and np.all(left[4 * len(s):] <= 70) and np.all(right[4 * len(s):] <= 70)
        pos, n = t2k.layout(left, right, parity)
        start = pos - left
        assert np.array_equal(start & 1, parity) and start[0] == 0 and np.all(start[1:] > (pos + right)[:-1])
        assert pos[-1] + right[-1] + 1 == n
        for L, R in s:
            rows = (left == L) & (right == R)
            assert {(int(f), int(p)) for f, p in zip(flag[rows], parity[rows])} >= {(0, 0), (0, 1), (1, 0), (1, 1)}
