"""BASELINE configs[0] ("C1") for real: the reference's OWN launcher (`gslam`, GSLAM/gslam/main.cpp) with its own `play`
and `metric_time` application plugins (GSLAM/plugins/play/main.cpp, GSLAM/evaluation/metric_time/main.cpp), all three
compiled unchanged from /root/reference (Makefile target `refapps`), runs

    gslam play orbhip metric_time -dataset seq.synthplane -slam orbhip ...

The dataset plugin (libgslamDB_synthplane.so, GSLAM_REGISTER_DATASET) renders a 640x480 monocular sequence of a textured
plane; the `orbhip` application extracts, matches to the previous frame, calls Optimizer::optimizePnP every frame and
Optimizer::optimize on a sliding window, and publishes "orbhip/curframe" / "orbhip/map"; `metric_time` measures the
per-frame latency between "dataset/frame" and "orbhip/curframe".  Everything the plugins computed is replayed through
the CPU oracle: keypoints / descriptors / matches bit-exact, PnP poses and the BA window within tolerance, and the
estimated trajectory must follow the dataset's ground truth."""
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "gslam_amd", "lib")
PLUGDIR = os.path.join(ROOT, "oracle", "_ref", "plugins")
REFDIR = os.path.join(ROOT, "oracle", "_ref", "apps")
W, H, K = 640, 480, 1000


def _need():
    for p in (os.path.join(REFDIR, "gslam"), os.path.join(REFDIR, "libgslam_play.so"),
              os.path.join(REFDIR, "libgslam_metric_time.so"), os.path.join(REFDIR, "libgslam_metric_traj.so"),
              os.path.join(PLUGDIR, "libgslam_orbhip.so"),
              os.path.join(PLUGDIR, "libgslamDB_synthplane.so")):
        if not os.path.exists(p):
            pytest.skip(f"{p} missing: `make plugins` builds it where the GSLAM headers are")


def _read_dump(path):
    raw = open(path, "rb").read()
    n, w, h = struct.unpack("3i", raw[:12])
    rec = 4 + 8 + 56 + w * h
    frames = {}
    for i in range((len(raw) - 12) // rec):
        o = 12 + i * rec
        fid = struct.unpack("i", raw[o:o + 4])[0]
        pose = np.frombuffer(raw, np.float64, 7, o + 12)
        img = np.frombuffer(raw, np.uint8, w * h, o + 68).reshape(h, w)
        frames[fid] = (pose, img)
    return frames


def _read_log(path):
    raw = open(path, "rb").read()
    o, out = 0, {"frames": [], "pnp": [], "ba": []}
    rd = lambda fmt: struct.unpack_from(fmt, raw, o)
    while o + 4 <= len(raw):
        typ = rd("i")[0]
        o += 4
        if typ == 1:
            fid, n = rd("2i")
            o += 8
            kps = np.frombuffer(raw, oracle_lib.KP_DTYPE, n, o).copy()
            o += 28 * n
            desc = np.frombuffer(raw, np.uint8, n * 32, o).reshape(n, 32).copy()
            o += 32 * n
            nm = rd("i")[0]
            o += 4
            m = np.frombuffer(raw, np.int32, 2 * nm, o).reshape(nm, 2).copy()
            o += 8 * nm
            out["frames"].append(dict(id=fid, kps=kps, desc=desc, matches=m))
        elif typ == 2:
            fid, n = rd("2i")
            o += 8
            xm = np.frombuffer(raw, np.float64, 5 * n, o).reshape(n, 5).copy()
            o += 40 * n
            start = np.frombuffer(raw, np.float64, 7, o).copy()
            pose = np.frombuffer(raw, np.float64, 7, o + 56).copy()
            o += 112
            ok = rd("i")[0]
            o += 4
            out["pnp"].append(dict(id=fid, X=xm[:, :3], m=xm[:, 3:], start=start, pose=pose, ok=ok))
        elif typ == 3:
            fid, nc, npt, no = rd("4i")
            o += 16
            poses, dof = np.zeros((nc, 7)), np.zeros(nc, np.int32)
            for c in range(nc):
                poses[c] = np.frombuffer(raw, np.float64, 7, o)
                dof[c] = struct.unpack_from("i", raw, o + 56)[0]
                o += 60
            pts = np.frombuffer(raw, np.float64, 3 * npt, o).reshape(npt, 3).copy()
            o += 24 * npt
            ocam, opt, oxy = np.zeros(no, np.int32), np.zeros(no, np.int32), np.zeros((no, 2))
            for k in range(no):
                ocam[k], opt[k] = struct.unpack_from("2i", raw, o)
                oxy[k] = np.frombuffer(raw, np.float64, 2, o + 8)
                o += 24
            ok = rd("i")[0]
            o += 4
            rposes = np.frombuffer(raw, np.float64, 7 * nc, o).reshape(nc, 7).copy()
            o += 56 * nc
            rpts = np.frombuffer(raw, np.float64, 3 * npt, o).reshape(npt, 3).copy()
            o += 24 * npt
            out["ba"].append(dict(id=fid, graph={"cam_pose": poses, "cam_dof": dof, "point_xyz": pts, "obs_cam": ocam,
                                                  "obs_point": opt, "obs_xy": oxy}, ok=ok, poses=rposes, pts=rpts))
        elif typ == 4:
            fid, nb = rd("2i")
            o += 8
            bw = np.frombuffer(raw, np.dtype([("id", "<u4"), ("v", "<f4")]), nb, o).copy()
            o += 8 * nb
            nf = rd("i")[0]
            o += 4
            feat = {}
            for _ in range(nf):
                node, cnt = struct.unpack_from("Ii", raw, o)
                o += 8
                feat[node] = np.frombuffer(raw, np.uint32, cnt, o).copy()
                o += 4 * cnt
            out.setdefault("bow", []).append(dict(id=fid, ids=bw["id"], vals=bw["v"], feat=feat))
        elif typ == 5:
            fid, nc = rd("2i")
            o += 8
            cands = []
            for _ in range(nc):
                cid, sc = struct.unpack_from("=id", raw, o)
                o += 12
                cands.append((cid, sc))
            loop_to, nm = rd("2i")
            o += 8
            m = np.frombuffer(raw, np.int32, 2 * nm, o).reshape(nm, 2).copy()
            o += 8 * nm
            out.setdefault("loops", []).append(dict(id=fid, cands=cands, loop_to=loop_to, matches=m))
        else:
            raise AssertionError(f"bad record type {typ} at {o}")
    return out


def _check_extraction_and_matches(oracle, frames, log):
    """Extraction + matching of every logged frame: bit-exact against the oracle on the frames the dataset delivered."""
    prev = None
    for f in log["frames"]:
        ek, ed = oracle.orb_extract(frames[f["id"]][1], K)
        assert len(ek) == len(f["kps"]) and f["kps"].tobytes() == ek.tobytes() and np.array_equal(f["desc"], ed)
        if prev is not None:
            fw = oracle.bf_match(ed, prev, threads=4)
            bw = oracle.bf_match(prev, ed, threads=4)
            keep = oracle.match_mask(fw[0], fw[1], fw[2], bw[0], len(prev), 100, 0, 1, 1).astype(bool)  # matchMaxDistance 100
            exp = np.stack([np.nonzero(keep)[0], fw[0][keep]], axis=1).astype(np.int32)
            assert np.array_equal(f["matches"], exp), f"matches of frame {f['id']}"
        else:
            assert len(f["matches"]) == 0
        prev = ed


def test_reference_launcher_runs_orbhip_on_the_synthetic_sequence(tmp_path, oracle):
    _need()
    n_frames = 45
    seq = tmp_path / "seq.synthplane"
    seq.write_text(f"width {W}\nheight {H}\nframes {n_frames}\nfps 200\ntexture 2048\nseed 1592590336\n"
                   f"dump {tmp_path / 'frames.bin'}\n")
    # Dataset::open -> Registry::load("gslamDB_synthplane") runs inside libgslam_play.so with THAT plugin's own svar
    # instance, whose search path is ".", /usr/lib ... (GSLAM/core/Registry.h:178-232): an installed GSLAM finds dataset
    # plugins in /usr/local/lib, here the plugin is linked into the working directory.
    os.symlink(os.path.join(PLUGDIR, "libgslamDB_synthplane.so"), tmp_path / "libgslamDB_synthplane.so")
    # Application order: the launcher starts each application's thread as soon as its plugin is loaded and keeps writing
    # svar["gslam"]["apps"] for the next one from the main thread (GSLAM/gslam/main.cpp:17-45) -- svar is not thread safe
    # (Svar.h:783), so `play`, which touches svar for its whole life, goes last.
    cmd = [os.path.join(REFDIR, "gslam"), "orbhip", "metric_time", "metric_traj", "play",
           "-dataset", str(seq), "-slam", "orbhip", "-playspeed", "1",
           "-orbhip.nFeatures", str(K), "-orbhip.log", str(tmp_path / "orbhip.bin"), "-orbhip.stop_on_finish", "1",
           "-orbhip.start_dataset", "1", "-orbhip.ba_every", "10", "-orbhip.ba_window", "8",
           "-FeatureDetectorPlugin", os.path.join(PLUGDIR, "libgslam_featuredetector.so"),
           "-OptimizerPlugin", os.path.join(PLUGDIR, "libgslam_optimizer.so"),
           "-GSLAM_LIBRARY_PATH", PLUGDIR + ":" + LIBDIR + ":" + REFDIR]
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = LIBDIR + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    # The reference launcher races on its global svar while applications start (see above); a crash in that window is the
    # launcher's, not the plugins': retry the run (observed: `play` listed first crashes every time, this order never).
    for attempt in range(3):
        for f in ("frames.bin", "orbhip.bin", "orbhip_metric_time.txt", "orbhip_traj_vo.txt", "orbhip_traj_final.txt"):
            if (tmp_path / f).exists():
                (tmp_path / f).unlink()
        r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=300, env=env)
        if r.returncode == 0 or r.returncode > 0:
            break
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]

    frames = _read_dump(tmp_path / "frames.bin")
    log = _read_log(tmp_path / "orbhip.bin")
    assert len(frames) == n_frames
    assert [f["id"] for f in log["frames"]] == list(range(1, n_frames + 1)), "a frame was lost between play and orbhip"

    # metric_time (the reference's evaluation plugin) saw every frame come back on "orbhip/curframe"
    mt = [ln.split() for ln in open(tmp_path / "orbhip_metric_time.txt").read().splitlines()]
    assert len(mt) == n_frames and all(0 < float(t) < 5.0 for _, t in mt)

    # metric_traj (the reference's trajectory evaluation plugin) consumed "orbhip/curframe" and "orbhip/map": one pose per
    # frame as published, and the map's frames (those that went through bundle adjustment last) sorted by id
    vo = np.loadtxt(tmp_path / "orbhip_traj_vo.txt")
    assert vo.shape == (n_frames, 8) and np.all(np.diff(vo[:, 0]) > 0)
    fin = np.loadtxt(tmp_path / "orbhip_traj_final.txt")
    assert fin.shape == (n_frames, 8) and np.allclose(fin[:, 0], vo[:, 0])

    _check_extraction_and_matches(oracle, frames, log)

    # optimizePnP twice on every frame but the first (robust fit, then refit on the inliers), replayed through the oracle
    assert [p["id"] for p in log["pnp"]] == [i for i in range(2, n_frames + 1) for _ in (0, 1)]
    for p in log["pnp"]:
        assert p["ok"] == 1 and len(p["X"]) >= 100
        po, so, _, rc = oracle.ba_pnp(p["X"], p["m"], p["start"], opts=oracle_lib.ba_options(huber=0.01, max_iterations=30))
        assert rc == 0 and np.abs(po - p["pose"]).max() <= 1e-8, p["id"]
    final = {p["id"]: p for p in log["pnp"]}  # the refit is the frame's pose

    # windowed bundle adjustment, replayed through the oracle
    assert len(log["ba"]) == n_frames // 10
    for b in log["ba"]:
        assert b["ok"] == 1 and len(b["graph"]["obs_cam"]) > 500
        eo = oracle.ba_solve(b["graph"], oracle_lib.ba_options(huber=0.01, max_iterations=30), threads=4)
        assert eo[3] == 0 and np.abs(eo[0] - b["poses"]).max() <= 1e-7 and np.abs(eo[1] - b["pts"]).max() <= 1e-7
        assert np.array_equal(b["poses"][:2], b["graph"]["cam_pose"][:2])  # the window's two oldest frames are the gauge

    # the tracked trajectory follows the renderer's ground truth: integer keypoints at pyramid scale localise a frame to
    # ~1 mm at 2.2 m from the plane, and frame-to-frame re-anchoring lets that accumulate (measured: 12 mm at most
    # over 45 frames; a scale-free window or unrejected outliers used to give 0.2 - 1 m)
    err = [np.linalg.norm(p["pose"][4:] - frames[i][0][4:]) for i, p in final.items()]
    assert max(err) < 0.03, max(err)
    q_err = [1 - abs(np.dot(p["pose"][:4], frames[i][0][:4])) for i, p in final.items()]
    assert max(q_err) < 1e-4
    # what metric_traj wrote is what the plugin calls produced: SE3 streams as "tx ty tz qx qy qz qw" (SE3.h operator<<);
    # the published pose of a frame is its PnP refit -- or, on the frames that close a BA window, the window's result for
    # its newest camera; the map's final pose of every frame additionally went through the later windows
    published = {i: p["pose"] for i, p in final.items()}
    for b in log["ba"]:
        published[b["id"]] = b["poses"][-1]
    for i, pose in published.items():  # the reference's Point3 / SO3 stream operators print 6 significant digits
        assert np.abs(vo[i - 1, 1:4] - pose[4:]).max() < 5e-6 and np.abs(vo[i - 1, 4:] - pose[:4]).max() < 5e-6, i
    assert np.abs(fin[:, 1:4] - np.array([frames[i + 1][0][4:] for i in range(n_frames)])).max() < 0.03


def test_launcher_bow_vectors_loop_candidates_and_connections(tmp_path, oracle):
    """`-orbhip.vocabulary voc.gbow`: every frame's BoW / feature vector through the Vocabulary plugin (libgslam_vocabulary,
    GPU transform) equals the oracle's on the logged descriptors; the loop candidates are the batched GPU scores of the
    frames at least `loop_gap` older, best first, equal to the oracle's scores; the orbit closes after 45 frames, so the last
    frames must find the first ones and verify them with node-consistent matches (a FrameConnection, "orbhip/loop")."""
    _need()
    from gslam_amd import bow_synth
    voc_lib = os.path.join(PLUGDIR, "libgslam_vocabulary.so")
    if not os.path.exists(voc_lib):
        pytest.skip("libgslam_vocabulary.so missing")
    n_frames, gap, levels_up = 45, 20, 2
    voc = bow_synth.make_vocabulary(k=10, L=4, seed=3)
    (tmp_path / "voc.gbow").write_bytes(bow_synth.to_gbow_bytes(voc))
    seq = tmp_path / "seq.synthplane"
    seq.write_text(f"width {W}\nheight {H}\nframes {n_frames}\nfps 200\ntexture 2048\nseed 1592590336\n")
    os.symlink(os.path.join(PLUGDIR, "libgslamDB_synthplane.so"), tmp_path / "libgslamDB_synthplane.so")
    cmd = [os.path.join(REFDIR, "gslam"), "orbhip", "metric_time", "play",
           "-dataset", str(seq), "-slam", "orbhip", "-playspeed", "1",
           "-orbhip.nFeatures", str(K), "-orbhip.log", str(tmp_path / "orbhip.bin"), "-orbhip.stop_on_finish", "1",
           "-orbhip.start_dataset", "1", "-orbhip.ba_every", "0",
           "-orbhip.vocabulary", str(tmp_path / "voc.gbow"), "-orbhip.loop_gap", str(gap), "-orbhip.levels_up", str(levels_up),
           "-orbhip.loop_score", "0.0", "-orbhip.loop_matches", "30",
           "-VocabularyPlugin", voc_lib,
           "-FeatureDetectorPlugin", os.path.join(PLUGDIR, "libgslam_featuredetector.so"),
           "-OptimizerPlugin", os.path.join(PLUGDIR, "libgslam_optimizer.so"),
           "-GSLAM_LIBRARY_PATH", PLUGDIR + ":" + LIBDIR + ":" + REFDIR]
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = LIBDIR + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    for attempt in range(3):
        for f in ("orbhip.bin", "orbhip_metric_time.txt"):
            if (tmp_path / f).exists():
                (tmp_path / f).unlink()
        r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=300, env=env)
        if r.returncode == 0 or r.returncode > 0:
            break
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = _read_log(tmp_path / "orbhip.bin")
    assert [f["id"] for f in log["frames"]] == list(range(1, n_frames + 1))
    assert [b["id"] for b in log["bow"]] == list(range(1, n_frames + 1)) == [lp["id"] for lp in log["loops"]]
    # metric_time saw the wrapped frames come back on "orbhip/curframe"
    assert len(open(tmp_path / "orbhip_metric_time.txt").read().splitlines()) == n_frames
    vecs = {}
    for f, b in zip(log["frames"], log["bow"]):
        word, weight, node, bw, bv = oracle.bow_transform(voc, f["desc"], levels_up)
        assert np.array_equal(b["ids"], bw) and np.array_equal(b["vals"], bv), f["id"]
        exp_feat = {}
        for i, nd in enumerate(node):
            if weight[i] > 0:  # a stop word (weight 0) enters neither vector (GSLAM/core/Vocabulary.h:1600-1612)
                exp_feat.setdefault(int(nd), []).append(i)
        assert sorted(b["feat"]) == sorted(exp_feat) and all(np.array_equal(b["feat"][k], np.array(v, np.uint32)) for k, v in exp_feat.items()), f["id"]
        vecs[f["id"]] = (bw, bv)
    descs = {f["id"]: f["desc"] for f in log["frames"]}
    nodes = {}
    for f in log["frames"]:
        word, weight, node, _, _ = oracle.bow_transform(voc, f["desc"], levels_up)
        nodes[f["id"]] = np.where(weight > 0, node.astype(np.int64), -1)  # a stop word is in no feature vector
    found = 0
    for lp in log["loops"]:
        old = [i for i in range(1, n_frames + 1) if i + gap <= lp["id"]]
        assert sorted(c[0] for c in lp["cands"]) == old
        sc = [c[1] for c in lp["cands"]]
        assert sc == sorted(sc, reverse=True)
        for cid, s in lp["cands"]:
            e = oracle.bow_score(int(voc["scoring"]), vecs[lp["id"]], vecs[cid])
            assert abs(s - e) <= 1e-6 * max(1.0, abs(e)), (lp["id"], cid, s, e)
        if not lp["cands"]:
            assert lp["loop_to"] == -1 and len(lp["matches"]) == 0
            continue
        # verification of the best candidate: cross-checked brute-force matches whose two features share their vocabulary node
        best = lp["cands"][0][0]
        q, t = descs[lp["id"]], descs[best]
        fw, bw_ = oracle.bf_match(q, t, threads=4), oracle.bf_match(t, q, threads=4)
        keep = oracle.match_mask(fw[0], fw[1], fw[2], bw_[0], len(t), 100, 0, 1, 1).astype(bool)
        qi = np.nonzero(keep)[0]
        ti = fw[0][keep]
        same = (nodes[lp["id"]][qi] >= 0) & (nodes[lp["id"]][qi] == nodes[best][ti])
        exp = np.stack([qi[same], ti[same]], axis=1).astype(np.int32)
        assert np.array_equal(lp["matches"], exp), lp["id"]
        assert lp["loop_to"] == (best if len(exp) >= 30 else -1), (lp["id"], len(exp))
        found += int(lp["loop_to"] >= 0)
    # (the procedural texture repeats, so the BoW scores of this sequence barely separate the frames: what is checked above
    #  is the machinery -- transform, batched scoring, ordering, node-consistent verification -- not place recognition)
    assert len([lp for lp in log["loops"] if lp["cands"]]) == n_frames - gap


def _launch_six_frames(tmp_path, options):
    """One launch of `gslam orbhip metric_traj play` on six frames of the synthetic sequence; returns the process, the
    frames the dataset dumped and the call log."""
    _need()
    seq = tmp_path / "seq.synthplane"
    seq.write_text(f"width {W}\nheight {H}\nframes 6\nfps 200\ntexture 2048\nseed 1592590336\n"
                   f"dump {tmp_path / 'frames.bin'}\n")
    os.symlink(os.path.join(PLUGDIR, "libgslamDB_synthplane.so"), tmp_path / "libgslamDB_synthplane.so")
    cmd = [os.path.join(REFDIR, "gslam"), "orbhip", "metric_traj", "play",
           "-dataset", str(seq), "-slam", "orbhip", "-playspeed", "1",
           "-orbhip.nFeatures", str(K), "-orbhip.log", str(tmp_path / "orbhip.bin"), "-orbhip.stop_on_finish", "1",
           "-orbhip.start_dataset", "1"] + options + [
           "-FeatureDetectorPlugin", os.path.join(PLUGDIR, "libgslam_featuredetector.so"),
           "-GSLAM_LIBRARY_PATH", PLUGDIR + ":" + LIBDIR + ":" + REFDIR]
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = LIBDIR + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r, _read_dump(tmp_path / "frames.bin"), _read_log(tmp_path / "orbhip.bin")


def test_lost_tracking_restarts_from_the_dataset_pose(tmp_path, oracle):
    """`-orbhip.min_track 100000` makes every frame with a predecessor in the window lose tracking: the window is cleared,
    the next frame starts again from the dataset's pose, so the window alternates between one frame and none, no
    optimizePnP and no optimize call is made, and every published frame still carries the dataset's pose."""
    r, frames, log = _launch_six_frames(tmp_path, [
        "-orbhip.min_track", "100000", "-orbhip.ba_every", "2", "-orbhip.ba_window", "3",
        "-OptimizerPlugin", os.path.join(PLUGDIR, "libgslam_optimizer.so")])
    assert sorted(frames) == list(range(1, 7))
    assert [f["id"] for f in log["frames"]] == list(range(1, 7))
    _check_extraction_and_matches(oracle, frames, log)
    assert log["pnp"] == [] and log["ba"] == []
    assert "bow" not in log and "loops" not in log
    vo = np.loadtxt(tmp_path / "orbhip_traj_vo.txt")
    assert vo.shape == (6, 8)
    for i in range(1, 7):  # "t tx ty tz qx qy qz qw", printed with 6 significant digits
        pose = frames[i][0]
        assert np.abs(vo[i - 1, 1:4] - pose[4:]).max() < 5e-6 and np.abs(vo[i - 1, 4:] - pose[:4]).max() < 5e-6, i


def test_track_off_extracts_and_matches_only(tmp_path, oracle):
    """`-orbhip.track 0`: no Optimizer plugin is loaded (none is even named); the application extracts, matches and
    publishes, and the log holds nothing but the frame records."""
    r, frames, log = _launch_six_frames(tmp_path, ["-orbhip.track", "0"])
    assert r.returncode == 0
    assert [f["id"] for f in log["frames"]] == list(range(1, 7))
    _check_extraction_and_matches(oracle, frames, log)
    assert log["pnp"] == [] and log["ba"] == []
    assert "bow" not in log and "loops" not in log
