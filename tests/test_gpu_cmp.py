"""GPU: the acoustic-composition kernels (magphase_cmp.hip: k_cmp_neighbours, k_cmp_compose, k_cmp_compose_bwd,
k_cmp_moment_tiles / k_cmp_moment_final) and mp.acoustic_compose_batch / mp.AcousticStats / la.interp_unv_regions with
their autograd, against tests/cmp_model.py.

Forward bound (derived): the kernel unit evaluates the model's float64 expressions in the model's order without fused
multiply-adds, so every stored element is the model's float64 value rounded to float32 -- held to ONE float32 ulp, nothing
excluded.  The neighbour table, the voicing column and the moments are held bit for bit.  The backward kernel is held to
(longest gap + 3 K + 2) x 2^-53 of sum |terms| against the model in the kernel's order.

Not derived (measured on the MI355X against the float64 model, pinned at <= 3 x the worst case, recorded through
_tol.within in profiles/r30_cmp_tolerance_report.json): the round trip against the original features and the gradients a
leaf receives (TOL below).  No frame and no column is left out of any comparison.

Shapes: F in {0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 257, 700}, utterances of 1, 2 and 70 frames side by side, every
voicing pattern of PATTERNS; unvoiced lf0 entries NaN, -1e10 or 0.0."""
import os

import numpy as np
import pytest
import torch

import cmp_model as cm
import mlpg_model as mm
from _tol import within
from magphase_amd import hostmath as hm
from magphase_amd import libaudio as la
from magphase_amd import magphase as mp

pytestmark = pytest.mark.gpu

FRAMES = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 257, 700)
SENT = -77.25
# measured on the MI355X (profiles/r30_cmp_tolerance_report.json), <= 3 x the worst case
TOL = {
    "roundtrip": 1.2e-7,        # |mlpg(compose(x)) - x|_inf / |x|_inf per stream and utterance (float32 rows)
    "roundtrip_norm": 1.1e-7,   # the same through norm= and its inverse
    "grad_f32": 1.1e-7,         # |leaf.grad - model|_inf / the largest sum |terms| of an element, float32 leaves
    "grad_f64": 6.5e-16,        # float64 leaves
    # through analysis_compressed_batch's backward against the torch float64 composition feeding the same backward: measured
    # 0 (both hand the analysis the same float32 bits), and a worst case of 0 cannot be scaled -- kept at one float32 ulp of
    # the upstream gradient (2^-23), the most the two float32 roundings of float64 values 2^-50 apart can differ by
    "grad_e2e": 2.0 ** -23,
}


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _ord32(a):
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def _ulps(got, want64):
    """Largest distance in float32 ulps between got (float32) and the float64 model value rounded to float32."""
    assert got.dtype == np.float32 and np.all(np.isfinite(got)), "a non-finite output"
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    return int(np.max(np.abs(_ord32(got) - _ord32(want)))) if got.size else 0


def _pattern(name, F, rng):
    m = np.zeros(F, dtype=bool)
    if name == "all":
        m[:] = True
    elif name == "first":
        m[:1] = True
    elif name == "middle":
        m[F // 2:F // 2 + 1] = True
    elif name == "last":
        m[F - 1:] = True
    elif name == "ends":
        m[:1] = True
        m[F - 1:] = True
    elif name == "alternating":
        m[::2] = True
    elif name == "straddle":          # gaps over a 64-lane tile edge and over a 256-frame pass, and a 300-frame gap
        m[:] = True
        for a, b in ((60, 70), (120, 130), (250, 262), (330, 630), (690, 700)):
            m[a:b] = False
        m[:3] = False
    elif name == "random":
        m = rng.random(F) < 0.5
    else:
        assert name == "none"
    return m


PATTERNS = ("all", "none", "first", "middle", "last", "ends", "straddle", "alternating", "random")


def _batch(dims, interp, unv, seed, dtype=np.float64, frames=None):
    """Per utterance the statics [F x SD] (float64 holding values of dtype; the carried column > 0 where voiced, `unv`
    elsewhere) -- every pattern at F = 700 and 257, the other frame counts with the patterns in turn, then 1, 2, 70."""
    rng = np.random.default_rng(seed)
    todo = [(700, p) for p in PATTERNS] + [(257, p) for p in PATTERNS]
    todo += [(F, PATTERNS[i % len(PATTERNS)]) for i, F in enumerate(FRAMES)] + [(1, "all"), (2, "last"), (70, "straddle")]
    if frames is not None:
        todo = [F if isinstance(F, tuple) else (F, PATTERNS[(i + seed) % len(PATTERNS)]) for i, F in enumerate(frames)]
    s0 = cm.offsets(dims)
    utts = []
    for F, p in todo:
        x = rng.normal(size=(F, s0[-1])).astype(dtype).astype(np.float64)
        if interp >= 0:
            c = s0[interp]
            x[:, c] = (4.0 + rng.random(F)).astype(dtype)
            x[~_pattern(p, F, rng), c] = unv
        utts.append(x)
    return utts


def _model(utts, dims, interp, vuv, windows, norm=None, fill=0.0):
    mean, std = norm if norm is not None else (None, None)
    return [cm.compose(x, dims, interp=interp, vuv=vuv, windows=windows, mean=mean, std=std, fill=fill) for x in utts]


def _norm(W, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=W), np.exp(rng.normal(size=W))


# ------------------------------------------------------------------------------------------------ kernels directly
@pytest.mark.parametrize("unv,xdt", ((np.nan, np.float64), (-1e10, np.float32), (0.0, np.float32)),
                         ids=("nan_f64", "magic_f32", "zero_f32"))
def test_kernels_directly(unv, xdt):
    e = _engine()
    dims, interp, vuv, windows = [3, 1, 2], 1, True, hm.mlpg_windows(cm.WINDOWS)
    utts = _batch(dims, interp, unv, 11, dtype=xdt)
    offs = np.concatenate(([0], np.cumsum([x.shape[0] for x in utts]))).astype(np.int64)
    total, SD, W, pad = int(offs[-1]), 6, 19, 2
    tdt = torch.float64 if xdt == np.float64 else torch.float32
    wide = torch.full((total, pad + SD + 3), float("nan"), dtype=tdt, device=e.device)       # NaN-fenced operand
    wide[:, pad:pad + SD] = torch.from_numpy(np.concatenate(utts)).to(e.device).to(tdt)
    x = wide[:, pad:pad + SD]
    offs_dev = torch.from_numpy(offs.astype(np.int32)).to(e.device)
    # the neighbour table inside a sentinel-filled buffer
    guard = 64
    nbuf = torch.full((guard + 2 * total + guard,), -7, dtype=torch.int32, device=e.device)
    nb = nbuf[guard:guard + 2 * total].view(2, total)
    assert e.cmp_neighbours(x[:, 3], offs_dev, out=nb) is nb
    h = nbuf.cpu().numpy()
    assert np.all(h[:guard] == -7) and np.all(h[guard + 2 * total:] == -7), "neighbours: written outside the table"
    want = [cm.voiced_neighbours(u[:, 3]) for u in utts]
    got = h[guard:guard + 2 * total].reshape(2, total)
    assert np.array_equal(got[0], np.concatenate([p for p, _ in want])), "prev"
    assert np.array_equal(got[1], np.concatenate([n for _, n in want])), "next"
    # the composition into a sentinel-filled pitched output, with and without norm
    for norm in (None, _norm(W, 5)):
        ld = W + 5
        obuf = torch.full((guard + total * ld + guard,), SENT, dtype=torch.float32, device=e.device)
        out = obuf[guard:guard + total * ld].view(total, ld)[:, :W]
        assert e.cmp_compose(x, nb, offs_dev, dims, interp, vuv, windows, norm=norm, unv_fill=-3.5, out=out) is out
        ho = obuf.cpu().numpy()
        assert np.all(ho[:guard] == SENT) and np.all(ho[guard + total * ld:] == SENT), "compose: written outside"
        body = ho[guard:guard + total * ld].reshape(total, ld)
        assert np.all(body[:, W:] == SENT), "compose: written beyond a row's last column"
        model = np.concatenate(_model(utts, dims, interp, vuv, cm.WINDOWS, norm, fill=-3.5))
        assert _ulps(np.ascontiguousarray(body[:, :W]), model) <= 1
        if norm is None:
            voiced = np.concatenate([p == np.arange(p.size) for p, _ in want])
            assert np.array_equal(body[:, W - 1], voiced.astype(np.float32)), "the voicing column"
    # the float64 output (la.interp_unv_regions' form) equals the model bit for bit
    o64 = e.cmp_compose(x, nb, offs_dev, dims, interp, vuv, windows, unv_fill=-3.5, out_f64=True).cpu().numpy()
    model = np.concatenate(_model(utts, dims, interp, vuv, cm.WINDOWS, None, fill=-3.5))
    assert np.all(np.isfinite(o64)) and np.max(np.abs(o64 - model)) <= 2.0 ** -52 * np.max(np.abs(model))


def test_backward_kernel_directly():
    e = _engine()
    dims, interp, vuv, windows = [2, 1, 2], 1, True, hm.mlpg_windows(cm.WINDOWS)
    utts = _batch(dims, interp, np.nan, 13, frames=((1, "all"), (2, "last"), (70, "straddle"), (0, "none"), (3, "middle"), (65, "alternating"),
                                                     (130, "ends"), (64, "first"), (129, "random"), (5, "none")))
    offs = np.concatenate(([0], np.cumsum([x.shape[0] for x in utts]))).astype(np.int64)
    total, SD, W = int(offs[-1]), 5, 16
    rng = np.random.default_rng(14)
    g = rng.normal(size=(total, W)).astype(np.float32)
    std = np.exp(rng.normal(size=W))
    x = torch.from_numpy(np.concatenate(utts)).to(e.device)
    offs_dev = torch.from_numpy(offs.astype(np.int32)).to(e.device)
    nb = e.cmp_neighbours(x[:, 2], offs_dev)
    gw = torch.full((total, W + 3), float("nan"), dtype=torch.float32, device=e.device)
    gw[:, :W] = torch.from_numpy(g).to(e.device)
    for sd in (None, std):
        gx = e.cmp_compose_backward(gw[:, :W], nb, offs_dev, dims, interp, vuv, windows, std=sd).cpu().numpy()
        assert gx.shape == (total, SD) and np.all(np.isfinite(gx))
        for u, xu in enumerate(utts):
            a, b = int(offs[u]), int(offs[u + 1])
            if b == a:
                continue
            want = cm.compose_backward(g[a:b], xu, dims, interp=interp, vuv=vuv, std=sd)
            scale = cm.compose_backward(np.abs(g[a:b]), xu, dims, interp=interp, vuv=vuv, windows=np.abs(cm.WINDOWS),
                                        std=sd)
            frac = np.max(np.abs(gx[a:b] - want) / np.maximum(scale, 1e-300)) / ((130 + 3 * 3 + 2) * 2.0 ** -53)
            within(frac, 1.0, "CMP_BWD_KERNEL_VS_MODEL_FRACTION")
            assert np.all(gx[a:b][np.isnan(xu)] == 0.0), "an unvoiced lf0 entry got a gradient"


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_moments_kernel_bit_for_bit(dtype):
    e = _engine()
    rng = np.random.default_rng(15)
    for total, W in ((1, 3), (127, 2), (128, 5), (129, 4), (700, 19)):
        x = (3.0 + rng.normal(size=(total, W)) * np.exp(rng.normal(size=W))).astype(dtype)
        wide = torch.full((total, W + 3), float("nan"), dtype=torch.from_numpy(x).dtype, device=e.device)
        wide[:, :W] = torch.from_numpy(x).to(e.device)
        obuf = torch.full((8 + 1 + 2 * W + 8,), SENT, dtype=torch.float64, device=e.device)
        out = obuf[8:8 + 1 + 2 * W]
        e.cmp_column_moments(wide[:, :W], out=out)
        h = obuf.cpu().numpy()
        assert np.all(h[:8] == SENT) and np.all(h[8 + 1 + 2 * W:] == SENT)
        n, sums, m2 = cm.column_moments(x)
        assert h[8] == n and np.array_equal(h[9:9 + W], sums) and np.array_equal(h[9 + W:9 + 2 * W], m2)
        assert torch.equal(e.cmp_column_moments(wide[:, :W]), out)          # the same bits on every run


# ------------------------------------------------------------------------------------------------ layouts, public API
LAYOUTS = {
    "default": (mp.MLPG_LAYOUT, True, cm.WINDOWS, np.float32),
    "lf0_alone": ((("lf0", 1),), True, cm.WINDOWS, np.float64),
    "lf0_first_of_three": ((("lf0", 1), ("a", 4), ("b", 2)), True, cm.WINDOWS, np.float64),
    "wide_65": ((("w", 65), ("lf0", 1)), True, cm.WINDOWS, np.float32),
    "no_lf0": ((("a", 5), ("b", 3)), False, cm.WINDOWS, np.float32),
    "no_vuv": ((("a", 5), ("lf0", 1)), False, cm.WINDOWS, np.float64),
    "one_window": ((("a", 5), ("lf0", 1)), True, cm.WINDOWS[:1], np.float32),
    "other_window": ((("a", 5), ("lf0", 1)), True, ((0.25, -0.5, 0.75),), np.float64),
}


def _split(x, dims):
    s0 = cm.offsets(dims)
    return tuple(x[:, a:b] if b - a > 1 else x[:, a] for a, b in zip(s0[:-1], s0[1:]))


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_layouts_host_and_device_inputs(name):
    layout, vuv, windows, dt = LAYOUTS[name]
    e = _engine()
    dims = [d for _, d in layout]
    interp = next((i for i, (n, _) in enumerate(layout) if n == "lf0"), -1)
    utts = _batch(dims, interp, -1e10, 21, dtype=dt, frames=(70, 1, 0, 2, 129, 3, 65))
    K = len(windows) + 1
    W = K * sum(dims) + int(vuv)
    norm = _norm(W, 22)
    model = _model(utts, dims, interp, vuv, windows, norm, fill=1.5)
    host = mp.acoustic_compose_batch([_split(x.astype(dt), dims) for x in utts], layout=layout, vuv=vuv, windows=windows,
                                     norm=norm, unv_fill=1.5)
    # device tensors: column slices of one wide matrix per utterance (lf0 a strided vector)
    tdt = torch.float64 if dt == np.float64 else torch.float32
    wides = [torch.cat([torch.full((x.shape[0], 2), float("nan"), dtype=tdt), torch.from_numpy(x).to(tdt)], 1).to(e.device)
             for x in utts]
    dev = mp.acoustic_compose_batch([_split(w[:, 2:], dims) for w in wides], layout=layout, vuv=vuv, windows=windows,
                                    norm=(torch.from_numpy(norm[0]).to(e.device), torch.from_numpy(norm[1]).to(e.device)),
                                    unv_fill=1.5, return_device=True)
    assert len(host) == len(dev) == len(utts)
    for h, d, m, x in zip(host, dev, model, utts):
        assert h.dtype == np.float64 and h.shape == (x.shape[0], W)
        assert d.dtype == torch.float32 and tuple(d.shape) == (x.shape[0], W) and d.grad_fn is None
        dh = d.cpu().numpy()
        assert np.array_equal(h, dh.astype(np.float64)), "host-array call != device-tensor call"
        assert _ulps(dh, m) <= 1
    assert dev[0].untyped_storage().data_ptr() == dev[-1].untyped_storage().data_ptr()      # views of one buffer


def test_bfloat16_streams_and_mixed_inputs():
    e = _engine()
    layout = (("a", 3), ("lf0", 1))
    utts = _batch([3, 1], 1, -1e10, 23, frames=(40, 5))
    bf = [torch.from_numpy(x).to(torch.bfloat16) for x in utts]
    utts = [b.double().numpy() for b in bf]
    model = _model(utts, [3, 1], 1, True, cm.WINDOWS)
    dev = mp.acoustic_compose_batch([(b[:, :3].to(e.device), b[:, 3].to(e.device)) for b in bf], layout=layout,
                                    return_device=True)
    mixed = mp.acoustic_compose_batch([(b[:, :3].to(e.device), x[:, 3]) for b, x in zip(bf, utts)], layout=layout,
                                      return_device=True)
    for d, mx, m in zip(dev, mixed, model):
        assert _ulps(d.cpu().numpy(), m) <= 1 and torch.equal(d, mx)
    single = mp.acoustic_compose(np.zeros((4, 60)), np.zeros((4, 10)), np.zeros((4, 10)), np.array([1.0, -1e10, 0.0, 3.0]))
    assert single.shape == (4, 244) and single[:, 243].tolist() == [1.0, 0.0, 0.0, 1.0]
    assert np.allclose(single[:, 240], [1.0, 1.0 + 2.0 / 3.0, 1.0 + 4.0 / 3.0, 3.0], rtol=1e-6)
    empty = mp.acoustic_compose_batch([(np.zeros((0, 3)), np.zeros(0))], layout=layout)
    assert empty[0].shape == (0, 13)


def test_deltas_equal_dynamic_features_of_the_carried_statics():
    dims = [4, 1]
    utts = _batch(dims, 1, np.nan, 24, frames=(70, 1, 2, 129, 64))
    rows = mp.acoustic_compose_batch([_split(x, dims) for x in utts], layout=(("a", 4), ("lf0", 1)), vuv=False,
                                     return_device=True)
    carried = []
    for x in utts:
        y = x.copy()
        y[:, 4] = cm.carried(x[:, 4], *cm.voiced_neighbours(x[:, 4]))
        carried.append(y)
    dyn_a = mp.dynamic_features_batch([y[:, :4] for y in carried])
    dyn_l = mp.dynamic_features_batch([y[:, 4:] for y in carried])
    for r, a, l in zip(rows, dyn_a, dyn_l):
        assert _ulps(r.cpu().numpy(), np.concatenate([a, l], axis=1)) <= 1


# ------------------------------------------------------------------------------------------------ round trip
def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b))) if b.size else 0.0


@pytest.mark.parametrize("with_norm", (False, True), ids=("plain", "norm"))
def test_round_trip_through_mlpg(with_norm):
    e = _engine()
    layout = mp.MLPG_LAYOUT
    dims = [d for _, d in layout]
    utts = _batch(dims, 3, la.MAGIC, 31, frames=(70, 1, 2, 129, 0, 5))
    W, K = 244, 3
    feats = [_split(x, dims) for x in utts]
    norm = _norm(W, 32) if with_norm else None
    rows = mp.acoustic_compose_batch(feats, norm=norm, return_device=True)
    if with_norm:
        mean, std = (torch.from_numpy(v).to(e.device) for v in norm)
        rows = [r.double() * std + mean for r in rows]
    back = mp.mlpg_streams_batch(rows, np.ones(W), return_device=True)
    _, streams, _ = hm.mlpg_layout(layout, True, K)
    label = "CMP_ROUNDTRIP_NORM" if with_norm else "CMP_ROUNDTRIP"
    for x, r, b in zip(utts, rows, back):
        F = x.shape[0]
        voiced = cm.voiced_mask(x[:, 80])
        rh = r.double().cpu().numpy()
        for s, ((c, d), (a0, a1)) in enumerate(zip(streams, zip(cm.offsets(dims)[:-1], cm.offsets(dims)[1:]))):
            got = b[s].cpu().numpy().reshape(F, d)
            if F == 0:
                continue
            # against the MLPG model fed the rows the device composed: the existing MLPG bounds
            mu = rh[:, c:c + K * d].reshape(F, K, d)
            if s == 3:
                traj = np.where(voiced, got[:, 0], 0.0)[:, None]
                ref_in = mp.mlpg_batch([rh[:, c:c + K * d]], np.ones(K * d))[0]           # the unmasked trajectory
                eta, fwd, _, _ = mm.band_errors(ref_in, mu, np.ones((F, K, d)))
                assert np.array_equal(got[~voiced, 0], np.full(int((~voiced).sum()), la.MAGIC)), "unvoiced lf0 != MAGIC"
                assert np.array_equal(got[voiced, 0], ref_in[voiced, 0])
                want, have = x[voiced, a0:a1], traj[voiced]
            else:
                eta, fwd, _, _ = mm.band_errors(got, mu, np.ones((F, K, d)))
                want, have = x[:, a0:a1], got
            within(float(np.max(eta)), 1.0, "CMP_ROUNDTRIP_MLPG_ETA_FRACTION")
            within(float(np.max(fwd)), 1.0, "CMP_ROUNDTRIP_MLPG_FORWARD_FRACTION")
            # against the original features
            if want.size:
                err = _rel(have, want)
                print("%s: stream %d F %d: %.4g" % (label, s, F, err))
                within(err, TOL["roundtrip_norm" if with_norm else "roundtrip"], label)


# ------------------------------------------------------------------------------------------------ la, statistics
def test_interp_unv_regions_equals_the_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "g18_interp_unv.npz"))
    batches = {}
    for i in range(int(g["ncases"])):
        data, voi, want = g["c%d_data" % i], g["c%d_voi" % i], g["c%d_out" % i]
        cond, kind = str(g["conds"][i]), str(g["kinds"][i])
        got = la.interp_unv_regions(data, voi, voi_cond=cond, interp_type=kind)
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.max(np.abs(got - want)) <= 1e-12, (i, cond, kind)
        poisoned = data.copy()
        poisoned[~hm.cmp_voi_cond(cond)[0](voi, hm.cmp_voi_cond(cond)[1])] = np.nan
        assert np.array_equal(la.interp_unv_regions(poisoned, voi, voi_cond=cond, interp_type=kind), got)
        batches.setdefault((cond, kind, data.ndim, data.shape[-1] if data.ndim == 2 else 0), []).append((data, voi, got))
    for (cond, kind, _nd, _n), items in batches.items():          # the one-launch form and device tensors
        e = _engine()
        outs = la.interp_unv_regions_batch([torch.from_numpy(d).to(e.device) for d, _, _ in items],
                                           [v for _, v, _ in items], voi_cond=cond, interp_type=kind)
        for o, (_, _, got) in zip(outs, items):
            assert np.array_equal(o, got)
    one = la.interp_unv_regions(np.array([np.nan, 2.5, np.nan]), np.array([0.0, 1.0, 0.0]))
    assert one.tolist() == [2.5, 2.5, 2.5]                        # one voiced row: held (the reference: NaN)


def test_acoustic_stats_three_uneven_batches_equal_one():
    e = _engine()
    rng = np.random.default_rng(41)
    W = 19
    mats = [(5.0 + rng.normal(size=(F, W)) * np.exp(rng.normal(size=W))).astype(np.float32) for F in (70, 1, 300, 129, 2, 64)]
    for m in mats:
        m[:, 7] = 1.25                                            # a zero-variance column ...
    one = mp.AcousticStats(W).update(mats)
    n, sums, m2 = cm.column_moments(np.concatenate(mats))
    assert one.n == n and np.array_equal(one.sums, sums) and np.array_equal(one.m2, m2)
    mean1, std1 = one.finalize()
    assert std1[7] == 1.0 and mean1[7] == 1.25                    # ... normalises to 0
    three = mp.AcousticStats(W)
    three.update(mats[:1]).update([torch.from_numpy(m).to(e.device) for m in mats[1:3]]).update(mats[3:])
    mean3, std3 = three.finalize()
    x = np.concatenate(mats).astype(np.float64)
    assert np.max(np.abs(mean3 - mean1) / np.abs(mean1)) <= 1e-12 and np.max(np.abs(std3 - std1) / std1) <= 1e-12
    assert np.max(np.abs(mean1 - x.mean(0)) / np.abs(x.mean(0))) <= 1e-12
    keep = np.arange(W) != 7
    assert np.max(np.abs(std1[keep] - x.std(0)[keep]) / x.std(0)[keep]) <= 1e-12
    rows = mp.acoustic_compose_batch([(m[:, :6].astype(np.float64), np.abs(m[:, 6]).astype(np.float64)) for m in mats],
                                     layout=(("a", 6), ("lf0", 1)), vuv=False, return_device=True)
    st = mp.AcousticStats(21).update(rows)                        # device rows as returned above
    normed = mp.acoustic_compose_batch([(m[:, :6].astype(np.float64), np.abs(m[:, 6]).astype(np.float64)) for m in mats],
                                       layout=(("a", 6), ("lf0", 1)), vuv=False, norm=st.finalize())
    z = np.concatenate(normed)
    assert np.max(np.abs(z.mean(0))) <= 1e-5 and np.max(np.abs(z.std(0) - 1.0)) <= 1e-5


# ------------------------------------------------------------------------------------------------ gradients
G_LAYOUT = (("a", 3), ("lf0", 1), ("b", 2))
G_DIMS = [3, 1, 2]


def _grad_utts():
    """40 frames: held start 0..4, voiced 5..10, gap 11..19, voiced 20..30, held end 31..39; and 1, 2, 7 frames."""
    rng = np.random.default_rng(51)
    utts = []
    for F, unvoiced in ((40, list(range(5)) + list(range(11, 20)) + list(range(31, 40))), (1, []), (2, [0]), (7, [3])):
        x = rng.normal(size=(F, 6)).astype(np.float32).astype(np.float64)
        x[:, 3] = (4.0 + rng.random(F)).astype(np.float32)
        x[unvoiced, 3] = la.MAGIC
        utts.append(x)
    return utts


def _leaf_feats(utts, dev, tdt):
    return [tuple(torch.from_numpy(np.ascontiguousarray(p)).to(tdt).to(dev).requires_grad_(True) for p in _split(x, G_DIMS))
            for x in utts]


def _model_grads(utts, norm, gs):
    out = []
    for x, g in zip(utts, gs):
        xt = torch.from_numpy(x).requires_grad_(True)
        y = cm.compose_torch(xt, G_DIMS, interp=1, vuv=True, mean=norm[0], std=norm[1], fill=0.25)
        y.backward(torch.from_numpy(g.astype(np.float64)))
        out.append(xt.grad.numpy())
    return out


def _grad_scales(utts, norm, gs):
    """Per utterance the largest sum |terms| of a gradient element (the model's backward on |g| with |taps|): what a
    gradient error is relative to -- the acceleration of a linear gap sends an exact zero made of cancelling terms."""
    return [float(np.max(cm.compose_backward(np.abs(g), x, G_DIMS, interp=1, vuv=True, windows=np.abs(cm.WINDOWS),
                                             std=norm[1]), initial=0.0)) for x, g in zip(utts, gs)]


def _check_grads(feats, utts, ref, scales, tdt, label):
    for f, x, r, scale in zip(feats, utts, ref, scales):
        got = np.concatenate([t.grad.cpu().double().numpy().reshape(x.shape[0], -1) for t in f], axis=1)
        for t, p in zip(f, _split(x, G_DIMS)):
            assert t.grad.dtype == tdt and tuple(t.grad.shape) == p.shape
        assert np.all(got[:, 3][x[:, 3] <= 0] == 0.0), "an unvoiced lf0 entry got a gradient"
        if scale > 0:
            err = float(np.max(np.abs(got - r))) / scale
            print("%s: F %d: %.4g" % (label, x.shape[0], err))
            within(err, TOL["grad_f64" if tdt == torch.float64 else "grad_f32"], label)
        else:
            assert not got.any() and not r.any()


@pytest.mark.parametrize("tdt", (torch.float32, torch.float64), ids=("f32", "f64"))
def test_gradients_match_the_float64_model(tdt):
    e = _engine()
    utts = _grad_utts()
    W = 19
    norm = _norm(W, 52)
    rng = np.random.default_rng(53)
    label = "CMP_GRAD_F64" if tdt == torch.float64 else "CMP_GRAD_F32"
    # a random upstream gradient, twice: the same bits
    gs = [rng.normal(size=(x.shape[0], W)).astype(np.float32) for x in utts]
    ref, scales = _model_grads(utts, norm, gs), _grad_scales(utts, norm, gs)
    runs = []
    for _ in range(2):
        feats = _leaf_feats(utts, e.device, tdt)
        rows = mp.acoustic_compose_batch(feats, layout=G_LAYOUT, norm=norm, unv_fill=0.25, return_device=True)
        assert all(r.grad_fn is not None and r.dtype == torch.float32 for r in rows)
        torch.autograd.backward(rows, [torch.from_numpy(g).to(e.device) for g in gs])
        _check_grads(feats, utts, ref, scales, tdt, label)
        runs.append([t.grad.clone() for f in feats for t in f])
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "two backward runs differ"
    # the forward values are the same bits with and without a grad_fn
    plain = mp.acoustic_compose_batch([tuple(t.detach() for t in f) for f in feats], layout=G_LAYOUT, norm=norm,
                                      unv_fill=0.25, return_device=True)
    assert all(p.grad_fn is None and torch.equal(p, r.detach()) for p, r in zip(plain, rows))
    # one-hot upstream gradients: first frame, last frame, inside the gap, in a held end (lf0 and another stream)
    for frame, col in ((0, 9), (0, 10), (39, 11), (39, 9), (15, 9), (15, 11), (35, 10), (2, 9), (0, 0), (39, 5), (20, 18)):
        gs = [np.zeros((x.shape[0], W), dtype=np.float32) for x in utts]
        gs[0][frame, col] = 1.0
        ref = _model_grads(utts, norm, gs)
        feats = _leaf_feats(utts, e.device, tdt)
        rows = mp.acoustic_compose_batch(feats, layout=G_LAYOUT, norm=norm, unv_fill=0.25, return_device=True)
        torch.autograd.backward(rows, [torch.from_numpy(g).to(e.device) for g in gs])
        _check_grads(feats, utts, ref, _grad_scales(utts, norm, gs), tdt, label + "_ONE_HOT")


def test_partial_gradients_and_no_grad_paths():
    e = _engine()
    utts = _grad_utts()[:1]
    feats = _leaf_feats(utts, e.device, torch.float32)
    only = [(feats[0][0].detach(), feats[0][1], utts[0][:, 4:6])]          # lf0 alone requires grad; a host stream
    rows = mp.acoustic_compose_batch(only, layout=G_LAYOUT, return_device=True)
    rows[0].sum().backward()
    assert feats[0][1].grad is not None and feats[0][0].grad is None
    with torch.no_grad():
        assert mp.acoustic_compose_batch(feats, layout=G_LAYOUT, return_device=True)[0].grad_fn is None
    host = mp.acoustic_compose_batch(feats, layout=G_LAYOUT)               # host result: no graph
    assert isinstance(host[0], np.ndarray)


def test_composes_with_the_compressed_analysis_backward():
    """A loss on the rows of analysis_compressed_batch(v_sig) reaches the samples.  A short synthetic utterance (the 37
    frames of the compressed analysis' own gradient tests) at 16 kHz with fft_len 1024: the compressed analysis has no
    mel-warp constant for 8 kHz (hostmath.define_alpha raises, as the reference's does), so this is the smallest case it
    runs."""
    import compressed_analysis_autograd_model as cam

    e = _engine()
    fs = cam.FS
    sig, pm_sec, voi = cam.batch_utts(1024)[1]          # 37 frames, voiced and unvoiced spacings mixed
    rng = np.random.default_rng(61)

    def run(dt):
        x = torch.from_numpy(sig).to(dt).to(e.device).requires_grad_(True)
        f = mp.analysis_compressed_batch([(x, fs, pm_sec, voi)], fft_len=1024, return_device=True)[0]
        rows = mp.acoustic_compose_batch([f[:4]], return_device=True)[0]
        return x, f, rows

    x, f, rows = run(torch.float32)
    assert rows.grad_fn is not None and rows.shape[1] == 244 and rows.shape[0] == f[0].shape[0]
    g = rng.normal(size=tuple(rows.shape)).astype(np.float32)
    rows.backward(torch.from_numpy(g).to(e.device))
    got = x.grad.cpu().double().numpy()
    assert got.shape == sig.shape and np.all(np.isfinite(got)) and np.any(got != 0)
    # the same chain by hand: the composition's own backward kernel (float64 out), then the analysis' backward
    x2 = torch.from_numpy(sig).to(e.device).requires_grad_(True)
    f2 = mp.analysis_compressed_batch([(x2, fs, pm_sec, voi)], fft_len=1024, return_device=True)[0]
    stat = torch.cat([f2[0].double(), f2[1].double(), f2[2].double(),
                      torch.from_numpy(np.asarray(f2[3], dtype=np.float64)).to(e.device)[:, None]], 1)
    y = cm.compose_torch(stat, [60, 10, 10, 1], interp=3, vuv=True)
    y.backward(torch.from_numpy(g.astype(np.float64)).to(e.device))
    ref = x2.grad.cpu().double().numpy()
    err = _rel(got, ref)
    print("CMP_GRAD_E2E: %.4g" % err)
    within(err, TOL["grad_e2e"], "CMP_GRAD_E2E")
