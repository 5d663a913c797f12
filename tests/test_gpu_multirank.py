"""
N > 1 code paths executed on ONE GPU (-m gpu): two ranks under torch.distributed.run share device 0 (gloo for the
barrier / reductions, BENCH_SHARE_DEVICE / MAGPHASE_SHARE_DEVICE for the device index).  What 8-GPU runs rely on:
bench.py's weak-scaling bookkeeping, the batch scripts' utterance sharding (files byte-identical to a single-process
run, nothing exchanged), mixed sample rates in one generation run, and per-utterance failure isolation.
"""
import json
import os
import socket
import subprocess
import sys
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return str(sk.getsockname()[1])


def _torchrun(nproc, script_args, extra_env, timeout=900):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=_free_port(), OMP_NUM_THREADS="4",
               HSA_ENABLE_IPC_MODE_LEGACY="0", **extra_env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % nproc,
           "--master-addr", "127.0.0.1", "--master-port", env["MASTER_PORT"]] + script_args
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_bench_two_ranks_on_one_device():
    one = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2", "--full", "--quick"],
                         cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert one.returncode == 0, one.stderr[-2000:]
    j1 = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    assert len(j1["per_rank"]) == 1
    # the N > 1 line carries the WHOLE contract: cpu_baseline, roofline with the fraction's spread
    # over the ranks, per_rank -- `BENCH_SHARE_DEVICE=1 python bench.py --gpus 2 --steps 20 --warmup 5 --full` (no e2e
    # block: the file-interface runs are covered by test_gpu_callers.py and take a minute)
    out = _torchrun(2, ["bench.py", "--gpus", "2", "--steps", "20", "--warmup", "5", "--full", "--no-e2e"],
                    {"BENCH_DIST_BACKEND": "gloo", "BENCH_SHARE_DEVICE": "1"}, timeout=1500)
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                             # rank 0 only
    j2 = json.loads(lines[0])
    assert j1["n_gpus"] == 1 and j2["n_gpus"] == 2 and j2["scaling"] == "weak"
    assert j2["config"]["frames_per_gpu"] > 0.9 * j1["config"]["frames_per_gpu"]
    # whole-job value = frames of BOTH ranks / max-over-ranks time: value * time == 2 ranks' frames
    f1 = j1["value"] * j1["ms_per_step"] * 1e-3
    f2 = j2["value"] * j2["ms_per_step"] * 1e-3
    assert abs(f1 - j1["config"]["frames_per_gpu"]) < 1e-3 * f1
    assert 1.9 * j1["config"]["frames_per_gpu"] < f2 < 2.1 * j1["config"]["frames_per_gpu"]
    cb, roof, pr = j2["cpu_baseline"], j2["roofline"], j2["per_rank"]
    assert cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] == "port"
    assert [r["rank"] for r in pr] == [0, 1]
    for r in pr:
        assert r["ms_per_step"] > 0 and r["kernel_ms"] > 0 and 0 < r["frac"] <= r["frac_8d"] < 1 and r["frames"] > 0
        assert r["ms_per_step"] <= j2["ms_per_step"] * 1.0001        # the line's time is the max over the ranks
    fr = roof["frac_ranks"]
    assert fr["min"] <= fr["mean"] <= fr["max"] and fr["min"] == min(r["frac"] for r in pr)
    # the headline fraction is the MOVED one (item 3); SURVEY 8d's figure is kept beside it
    assert abs(roof["frac"] - roof["moved_bytes"] / (roof["kernels"][0]["ms"] * 1e-3) / 1e9 / roof["peak"]) < 2e-3
    assert roof["frac_8d"] >= roof["frac"] and roof["alg_bytes_8d"] >= roof["moved_bytes"]
    assert "configs2" in j2 and "ms_per_step" in j2["configs2"]
    # host hygiene: every rank on its own cores, its native threads capped by them, and the host side
    # of a launch measured with all ranks at once against rank 0 alone
    hc = j2["host_contention"]
    assert hc["cores_bound"] and hc["ms_rank0_alone"] > 0 and hc["ms_max_over_ranks"] > 0
    assert hc["ratio_together_over_alone"] is not None and hc["ratio_together_over_alone"] < 2.0
    ncpu = len(os.sched_getaffinity(0))
    for r in pr:
        assert 1 <= r["native_threads_cap"] <= r["host_cores"] <= max(1, ncpu // 2) + 1 and r["host_prepare_ms"] > 0
    # the headline is one step at a time on one stream; the overlapped figure and the two-launch form stand beside it
    assert j2["config"]["streams"] == 1 and j2["value_overlapped"] >= 0.9 * j2["value"]
    # (no ordering between the two forms here: two ranks share ONE device in this test and either form can lose a turn)
    assert j2["value_two_launch"] > 0 and j2["config"]["other_form"]["ms_per_step"] > 0


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it starts two ranks itself (a bare
    `--gpus 8` used to run one rank and print n_gpus 1).  Both ranks share device 0 here; gloo carries the barrier."""
    env = dict(os.environ, BENCH_DIST_BACKEND="gloo", BENCH_SHARE_DEVICE="1", OMP_NUM_THREADS="4")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "5", "--warmup", "2", "--quick"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and "utterance-sharded x2" in j["config"]["parallelism"]
    f = j["value"] * j["ms_per_step"] * 1e-3
    assert 1.9 * j["config"]["frames_per_gpu"] < f < 2.1 * j["config"]["frames_per_gpu"]
    # the corpus workload through the same self-launch (strong scaling: the corpus is sharded over the ranks)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--workload", "corpus", "--utts", "48"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["n_gpus"] == 2 and j["scaling"] == "strong"


def test_bench_falls_back_to_gloo_when_rccl_cannot_initialise():
    """Two ranks on ONE device with the default backend: RCCL refuses ("duplicate GPU": ncclInvalidUsage) -- nothing on the
    data path needs it, so the run carries on over gloo instead of dying (multi-GPU weak points)."""
    env = dict(os.environ, BENCH_SHARE_DEVICE="1", OMP_NUM_THREADS="4")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "BENCH_DIST_BACKEND"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "5", "--warmup", "2", "--quick"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "falling back to gloo" in r.stderr
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["n_gpus"] == 2


def test_bench_refuses_more_ranks_than_devices():
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "BENCH_SHARE_DEVICE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "64", "--quick"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2 and "device(s) visible" in r.stderr


def _make_corpus(tmp_path, n, fs_list):
    sys.path.insert(0, os.path.join(ROOT, "demos"))
    import make_demo_data
    from magphase_amd import libaudio as la, synthetic as syn
    wav_dir = tmp_path / "wavs"
    os.makedirs(str(wav_dir), exist_ok=True)
    toks = []
    for u in range(n):
        fs = fs_list[u % len(fs_list)]
        pcm, pm, voi = syn.make_utterance(500 + u, dur_s=0.6 + 0.1 * (u % 3), fs=fs)
        tok = "m%02d" % u
        la.write_audio_file(str(wav_dir / (tok + ".wav")), pcm / 32768.0, fs, norm=None)
        make_demo_data.write_est(str(wav_dir / (tok + ".est")), pm, voi)
        toks.append((tok, fs))
    scp = tmp_path / "list.scp"
    scp.write_text("\n".join(t for t, _ in toks) + "\n")
    return str(wav_dir), str(scp), toks


def _same_files(d1, d2, names):
    for n in names:
        a, b = open(os.path.join(d1, n), "rb").read(), open(os.path.join(d2, n), "rb").read()
        assert len(a) > 0 and a == b, n


def test_batch_scripts_two_ranks_write_the_same_files_as_one_process(tmp_path):
    wav_dir, scp, toks = _make_corpus(tmp_path, 7, [48000])
    ext = os.path.join(ROOT, "scripts", "batch_feature_extraction_for_tts.py")
    gen = os.path.join(ROOT, "scripts", "batch_waveform_generation.py")
    p1, p2, g1, g2 = (str(tmp_path / d) for d in ("p1", "p2", "g1", "g2"))
    env = dict(os.environ)
    r = subprocess.run([sys.executable, ext, "--scp", scp, "--wav-dir", wav_dir, "--out-dir", p1, "--batch", "3"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    _torchrun(2, [ext, "--scp", scp, "--wav-dir", wav_dir, "--out-dir", p2, "--batch", "2"], {"MAGPHASE_SHARE_DEVICE": "1"})
    feat_names = [t + e for t, _ in toks for e in (".mag", ".real", ".imag", ".lf0", ".shift")]
    _same_files(p1, p2, feat_names)                        # batching and sharding do not change a bit of the features
    # --rank-subdirs: every rank creates its files in OUT_DIR/rank<r>/ (file creation in one directory serialises on its
    # lock: tools/file_interface_nproc.py, 8 processes: 20 700 x -> 91 000 x real time); same bytes, every token once
    p3 = str(tmp_path / "p3")
    _torchrun(2, [ext, "--scp", scp, "--wav-dir", wav_dir, "--out-dir", p3, "--batch", "2", "--rank-subdirs"],
              {"MAGPHASE_SHARE_DEVICE": "1"})
    found = {}
    for r_ in (0, 1):
        for n in os.listdir(os.path.join(p3, "rank%d" % r_)):
            assert n not in found
            found[n] = os.path.join(p3, "rank%d" % r_, n)
    assert sorted(found) == sorted(feat_names)
    for n in feat_names:
        assert open(found[n], "rb").read() == open(os.path.join(p1, n), "rb").read(), n
    common = ["--scp", scp, "--feats-dir", p1, "--mag-dim", "60", "--phase-dim", "10", "--pf-type", "magphase", "--noise", "device"]
    r = subprocess.run([sys.executable, gen] + common + ["--out-dir", g1, "--batch", "4"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    _torchrun(2, [gen] + common + ["--out-dir", g2, "--batch", "2"], {"MAGPHASE_SHARE_DEVICE": "1"})
    for t, _fs in toks:   # device noise is seeded by the token: same wav up to 1 LSB (run partition differs with the batch)
        with wave.open(os.path.join(g1, t + ".wav"), "rb") as w1, wave.open(os.path.join(g2, t + ".wav"), "rb") as w2:
            a = np.frombuffer(w1.readframes(w1.getnframes()), dtype=np.int16).astype(np.int32)
            b = np.frombuffer(w2.readframes(w2.getnframes()), dtype=np.int16).astype(np.int32)
        assert a.size == b.size and a.size > 20000 and np.max(np.abs(a - b)) <= 1, t


def test_mixed_sample_rates_and_failure_isolation(tmp_path):
    """configs[4]: 16 kHz and 48 kHz tokens in one generation run; a token with a truncated file and a missing wav do
    not stop the corpus and land in crash_file_list_<host>_<pid>.scp."""
    from magphase_amd import iobatch
    wav_dir, _scp, toks = _make_corpus(tmp_path, 6, [48000, 16000])
    wavs = [os.path.join(wav_dir, t + ".wav") for t, _ in toks]
    with open(os.path.join(wav_dir, "broken.wav"), "wb") as fh:
        fh.write(b"RIFF not a wav")
    feats = str(tmp_path / "feats")
    rep = iobatch.CorpusReport()
    iobatch.extract_features_corpus(wavs[:3] + [os.path.join(wav_dir, "broken.wav"), os.path.join(wav_dir, "absent.wav")] + wavs[3:],
                                    feats, batch_utts=4, phase_dim=45, verbose=False, report=rep)
    assert rep["done"] == 6 and sorted(t for t, _m in rep["failed"]) == ["absent", "broken"]
    assert open(rep["crash_list"]).read().split() == ["broken", "absent"]
    for t, _fs in toks:
        assert os.path.getsize(os.path.join(feats, t + ".mag")) > 0
    # generation with a token -> fs map; one token has a truncated .real file
    with open(os.path.join(feats, toks[1][0] + ".real"), "r+b") as fh:
        fh.truncate(45 * 4 * 3 + 2)
    out = str(tmp_path / "syn")
    rep2 = iobatch.CorpusReport()
    iobatch.generate_waveforms_corpus(feats, [t for t, _ in toks], out, 60, 45, dict(toks), pf_type="no", batch_utts=6,
                                      verbose=False, report=rep2, noise_mode="device")
    assert [t for t, _m in rep2["failed"]] == [toks[1][0]] and rep2["done"] == 5
    for t, fs in toks:
        if t == toks[1][0]:
            continue
        with wave.open(os.path.join(out, t + ".wav"), "rb") as w:
            assert w.getframerate() == fs and w.getnframes() > 0.4 * fs


def test_corpus_workload_two_ranks_on_one_device():
    """bench.py --workload corpus (BASELINE configs[3] + configs[4]): the 2-rank job processes exactly the corpus of the
    1-rank job (same frames, same audio), LPT-sharded, every utterance once; ONE JSON line from rank 0."""
    n = 96
    one = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--workload", "corpus", "--utts", str(n)], cwd=ROOT,
                         capture_output=True, text=True, timeout=900)
    assert one.returncode == 0, one.stderr[-3000:]
    j1 = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    out = _torchrun(2, ["bench.py", "--gpus", "2", "--workload", "corpus", "--utts", str(n)],
                    {"BENCH_DIST_BACKEND": "gloo", "BENCH_SHARE_DEVICE": "1"})
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j2 = json.loads(lines[0])
    assert j1["n_gpus"] == 1 and j2["n_gpus"] == 2 and j2["scaling"] == "strong"
    for key in ("configs3_extraction", "configs4_generation"):
        a, b = j1["corpus"][key], j2["corpus"][key]
        assert sum(b["per_rank_utts"]) == n and a["per_rank_utts"] == [n]
        assert min(b["per_rank_utts"]) >= n // 2 - 8                       # LPT: both ranks busy
        assert abs(b["audio_s"] - a["audio_s"]) < 0.2 and b["lpt_cost_imbalance_max_over_mean"] < 1.02
        # base utterances are seeded per rank, so the frame counts of the two jobs agree to a few percent, not exactly
        assert abs(b["frames"] - a["frames"]) < 0.05 * a["frames"] and b["frames_per_s"] > 0
    assert j2["value"] > 0 and j2["config"]["x_realtime"] > 50


def test_whole_10k_corpus_on_one_gpu():
    """
    BASELINE configs[3] + configs[4] at their FULL size on one device (the only BASELINE size no
    driver-run test had touched): the 10 000-utterance corpus of tools/corpus_workload.py (2-8 s utterances; extraction at
    48 kHz, 60 / 10, Q7; generation from perturbed features, 60 / 45, post-filter + output high-pass + 16-bit PCM, 48 kHz
    and 16 kHz MIXED), in 64-utterance launches through the batch API, as scripts/batch_feature_extraction_for_tts.py:40-57
    and scripts/batch_waveform_generation.py:28-58 run it.  Size-independent properties on EVERY utterance -- each one
    produced exactly once, frame counts / output lengths equal to the host plan (numpy planners, not the native batch
    planner the product used), finite values in range -- and three utterances per sample rate against the oracle (features;
    waveform with the noise draw the batch made for that utterance).
    """
    import warnings

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import corpus_workload as cw
    from _tol import within
    from magphase_amd import engine as em, hostmath as hm, magphase as mp
    from oracle import magphase_oracle as orc

    n = 10000
    batches = [np.arange(i, min(i + cw.BATCH, n)) for i in range(0, n, cw.BATCH)]
    picked = (0, len(batches) // 2, len(batches) - 1)         # launches whose first utterance per rate meets the oracle
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # ---------------- configs[3]: feature extraction, 48 kHz
        dur, fs_all = cw.corpus_spec(n, False)
        pool = cw._pool(0, 48000)
        seen, frames = np.zeros(n, dtype=int), np.zeros(n, dtype=int)
        n_oracle = 0
        for bi, idx in enumerate(batches):
            items = [cw._cut(pool[int(u) % cw.POOL], float(dur[u]), 48000) for u in idx]
            res = mp.analysis_compressed_batch(items, mag_dim=60, phase_dim=10, alpha_phase=False, as_float32=True)
            assert len(res) == len(idx)
            for u, it, r in zip(idx, items, res):
                seen[u] += 1
                frames[u] = r[0].shape[0]
                pm_s, voi_c = hm.clean_epochs(it[2], it[3], check_len_smpls=len(it[0]), fs=48000)   # the host plan, in numpy
                assert r[0].shape == (len(pm_s), 60) and r[1].shape == r[2].shape == (len(pm_s), 10)
                assert len(r[3]) == len(r[4]) == len(pm_s) and r[5] == 48000 and r[6] == 4096
                assert np.all(np.isfinite(r[0])) and max(np.max(np.abs(r[1])), np.max(np.abs(r[2]))) <= 1.0
            if bi in picked:
                pcm, fs, pm, voi = items[0]
                o = orc.analysis_compressed_from_epochs(pcm.astype(np.float64) / 32768.0, fs, pm, voi, mag_dim=60, phase_dim=10,
                                                        alpha_phase=False)
                assert np.array_equal(res[0][4], o[4]) and np.array_equal(res[0][3], o[3])
                within(np.max(np.abs(res[0][0] - o[0])), 1e-5, "CORPUS10K_FUSED_MAG")
                within(max(np.max(np.abs(res[0][1] - o[1])), np.max(np.abs(res[0][2] - o[2]))), 2e-6, "CORPUS10K_FUSED_PHASE")
                n_oracle += 1
        assert np.all(seen == 1) and n_oracle == 3
        assert 150 * dur.sum() < frames.sum() < 260 * dur.sum()           # ~175-200 pitch-synchronous frames per second

        # ---------------- configs[4]: waveform generation, 48 kHz (even utterances) and 16 kHz (odd) mixed
        dur, fs_all = cw.corpus_spec(n, True)
        rng = np.random.RandomState(777)
        feats = {}
        for rate in (16000, 48000):
            pool = cw._pool(0, rate)
            res = []
            for b in cw._batches([(p[0], rate, p[1], p[2]) for p in pool]):
                res += mp.analysis_compressed_batch(b, mag_dim=60, phase_dim=45, as_float32=True)
            feats[rate] = [(r[0] + rng.normal(0, 0.05, r[0].shape).astype(np.float32),
                            np.clip(r[1] + rng.normal(0, 0.05, r[1].shape).astype(np.float32), -1, 1),
                            np.clip(r[2] + rng.normal(0, 0.05, r[2].shape).astype(np.float32), -1, 1), r[3]) for r in res]
        seen, n_oracle = np.zeros(n, dtype=int), {16000: 0, 48000: 0}
        np.random.seed(4242)
        for bi, idx in enumerate(batches):
            for rate in (16000, 48000):
                grp = [int(u) for u in idx if int(fs_all[u]) == rate]
                if not grp:
                    continue
                group = []
                for u in grp:
                    m, re_, im, lf0 = feats[rate][u % cw.POOL]
                    k = max(8, int(round(m.shape[0] * float(dur[u]) / cw.BASE_DUR_S)))
                    group.append((m[:k], re_[:k], im[:k], lf0[:k]))
                state = np.random.get_state()                 # the launch draws its first utterance's noise from here
                sigs = mp.synthesis_from_compressed_batch(group, rate, b_out_hpf=True, b_post_filter=True, pcm16_norm=0.98)
                assert len(sigs) == len(grp)
                N = 4096 if rate == 48000 else 2048
                plan = em.plan_synthesis_numpy([g[3] for g in group], rate, N, False, True)      # numpy planner, per utterance
                for u, s, ln in zip(grp, sigs, plan["out_len"]):
                    seen[u] += 1
                    assert s.dtype == np.int16 and s.shape == (int(ln),)
                    assert 32100 <= int(np.max(np.abs(s.astype(np.int32)))) <= 32120       # 0.98 of full scale at the peak
                if bi in picked:
                    m, re_, im, lf0 = (np.asarray(a, dtype=np.float64) for a in group[0])
                    now = np.random.get_state()
                    np.random.set_state(state)
                    ref = orc.synthesis_from_compressed(orc.post_filter(m, rate), re_, im, lf0, rate, b_out_hpf=True)
                    np.random.set_state(now)
                    assert len(ref) == len(sigs[0])
                    # libsndfile's float -> 16-bit conversion (what la.write_audio_file / mpx_pcm16 do): x * 32767, rounded --
                    # half an LSB of rounding + the float path's 3e-7 of the peak (measured 0.52)
                    within(np.max(np.abs(sigs[0].astype(np.float64) - 32767.0 * orc.normalise_for_wav(ref, 0.98))),
                           0.75, "CORPUS10K_PCM16_LSB")
                    n_oracle[rate] += 1
        assert np.all(seen == 1) and n_oracle == {16000: 3, 48000: 3}
