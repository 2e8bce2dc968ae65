"""bench.py --dump-outputs: the arrays written for output-for-output comparison of two builds.  `dump_outputs` is run here on
CPU tensors shaped like the timed step's outputs: float32 / float64 only, under 64 MB, the same seeded sample every time, and
the entries past a frame's keypoint count written as fixed values."""
import os

import numpy as np
import torch

from test_bench_line import _bench


def _outputs(F, K, seed):
    g = torch.Generator().manual_seed(seed)
    kps = torch.rand((F, K, 7), generator=g)
    kps[..., 5:] = torch.randint(0, 8, (F, K, 2), generator=g, dtype=torch.int32).view(torch.float32)
    desc = torch.randint(0, 256, (F, K, 32), generator=g, dtype=torch.uint8)
    counts = torch.randint(K // 2, K + 1, (F,), generator=g, dtype=torch.int32)
    pq = torch.arange(F - 1, dtype=torch.int32)
    idx = torch.randint(-1, K, (F - 1, K), generator=g, dtype=torch.int32)
    d1 = torch.randint(0, 257, (F - 1, K), generator=g, dtype=torch.int16)
    d2 = torch.randint(0, 257, (F - 1, K), generator=g, dtype=torch.int16)
    return (kps, desc, counts), (idx, d1, d2), counts, pq, pq + 1


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_float_bounded_and_repeatable(tmp_path):
    bench = _bench()
    args = _outputs(200, 500, 1)
    bench.dump_outputs(str(tmp_path / "a"), *args)
    bench.dump_outputs(str(tmp_path / "b"), *_outputs(200, 500, 1))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == {"counts", "sample_frames", "keypoints", "descriptors", "sample_pairs", "match_idx", "match_d1", "match_d2"}
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    (kps, desc, counts), (idx, d1, _), _, pq, _ = args
    fs = a["sample_frames"].astype(np.int64)
    assert len(fs) == 64 and np.array_equal(a["counts"], counts.numpy())
    for i, f in enumerate(fs):
        c = int(counts[f])
        assert np.array_equal(a["descriptors"][i, :c], desc[f, :c].numpy()) and not a["descriptors"][i, c:].any()
        assert np.array_equal(a["keypoints"][i, :c, :5], kps[f, :c, :5].numpy())
        assert np.array_equal(a["keypoints"][i, :c, 5:], kps[f, :c, 5:].contiguous().view(torch.int32).numpy())
        assert not a["keypoints"][i, c:].any()
    for i, (q, t) in enumerate(a["sample_pairs"].astype(np.int64)):
        assert t == q + 1
        c = int(counts[q])
        assert np.array_equal(a["match_idx"][i, :c], idx[q, :c].numpy()) and (a["match_idx"][i, c:] == -1).all()
        assert np.array_equal(a["match_d1"][i, :c], d1[q, :c].numpy().view(np.uint16))


def test_dump_shrinks_the_sample_to_the_size_cap(tmp_path):
    bench = _bench()
    bench.dump_outputs(str(tmp_path), *_outputs(80, 40000, 2))
    a = _load(tmp_path)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert 1 <= len(a["sample_frames"]) < 64
