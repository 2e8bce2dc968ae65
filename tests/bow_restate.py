"""A plain numpy restatement of the BoW transform and the six scorings, written for the adversarial suites
(tests/test_bow_adversarial_oracle.py, tests/test_bow_adversarial_gpu.py).  It shares no code with oracle/bow_oracle.c or
the kernels: the census of tests/bow_cases.py is taken with it, and the oracle is then held to it.

  descent   np.unpackbits popcounts (binary) or a sequential np.float32 sum over the components (float), children
            p*k+1 .. p*k+childNum, first strict minimum (np.argmin returns the first), stop at childNum == 0; a float
            descent also stops where no child compares below FLT_MAX
  assembly  feature-order np.float32 adds for TF_IDF / TF, first weight for IDF / BINARY, w <= 0 skipped
  norms     double, ascending word id
  scores    float32 terms accumulated into one float64 in ascending id order (np.cumsum adds sequentially); KL takes
            np.log on float32
numpy only."""
import numpy as np

FLT_MAX = np.float32(3.402823466e+38)
LOG_EPS = np.log(np.finfo(np.float64).eps)


def _hamming(q, t):
    """q: m x W, t: m x c x W (uint8) -> m x c popcounts of the xor."""
    return np.unpackbits(q[:, None, :] ^ t, axis=2).sum(axis=2, dtype=np.int64)


def _l2_f32(q, t):
    """q: m x D, t: m x c x D float32 -> m x c squared L2, accumulated component by component in float32."""
    acc = np.zeros(t.shape[:2], np.float32)
    with np.errstate(all="ignore"):
        for e in range(q.shape[1]):
            tmp = q[:, None, e] - t[:, :, e]
            acc = acc + tmp * tmp
    return acc


def descend(voc, desc, levelsup, chunk=2048):
    """-> dict(word, weight, node, reached, end_level, tie, tie_first, tie_later).

    reached[i]: the descent of feature i wrote the node output (its level L - levelsup was visited, or that level is <= 0).
    tie[i]: at one level or more, two or more children were exactly at the minimum distance; tie_first / tie_later: at
    such a level the winner was the node's first child / a later child."""
    k, L = int(voc["k"]), int(voc["L"])
    child_num = voc["nodes"]["childNum"].astype(np.int64)
    nd = voc["desc"]
    is_float = nd.dtype == np.float32
    n = len(desc)
    word = np.zeros(n, np.int64)
    nid = np.zeros(n, np.int64)
    nid_level = L - levelsup
    reached = np.full(n, nid_level <= 0)
    end_level = np.zeros(n, np.int64)
    tie, tie_first, tie_later = (np.zeros(n, bool) for _ in range(3))
    active = np.ones(n, bool)
    level = 0
    while active.any():
        level += 1
        for s in range(0, n, chunk):
            idx = s + np.nonzero(active[s:s + chunk])[0]
            if not len(idx):
                continue
            p = word[idx]
            cn = child_num[p]
            cmax = int(cn.max())
            if cmax == 0:  # a root without children: the loop body runs once and changes nothing
                active[idx] = False
                end_level[idx] = level
                if level == nid_level:
                    reached[idx] = True
                continue
            kids = p[:, None] * k + 1 + np.arange(cmax)[None, :]
            valid = np.arange(cmax)[None, :] < cn[:, None]
            kid_desc = nd[np.where(valid, kids, 0)]
            if is_float:
                d = _l2_f32(desc[idx], kid_desc)
                with np.errstate(invalid="ignore"):
                    ok = valid & (d < FLT_MAX)
                d = np.where(ok, d, np.float32(np.inf))
            else:
                d = _hamming(desc[idx], kid_desc)
                ok = valid
                d = np.where(ok, d, 1 << 40)
            moved = ok.any(axis=1)
            best = np.argmin(d, axis=1)
            dmin = d[np.arange(len(idx)), best]
            ntie = (ok & (d == dmin[:, None])).sum(axis=1)
            t = moved & (ntie > 1)
            tie[idx] |= t
            tie_first[idx] |= t & (best == 0)
            tie_later[idx] |= t & (best > 0)
            mi = idx[moved]
            word[mi] = kids[moved, best[moved]]
            end_level[mi] = level
            if level == nid_level:
                nid[mi] = word[mi]
                reached[mi] = True
            active[idx[~moved]] = False
            active[mi] = child_num[word[mi]] != 0
    node = np.zeros(n, np.int64) if nid_level <= 0 else nid
    return dict(word=word.astype(np.uint32), weight=voc["nodes"]["weight"][word].astype(np.float32),
                node=node.astype(np.uint32), reached=reached, end_level=end_level, tie=tie, tie_first=tie_first,
                tie_later=tie_later)


def assemble(voc, word, weight):
    """-> (ids ascending uint32, values float32) of the image's BoW vector."""
    weighting, scoring = int(voc["weighting"]), int(voc["scoring"])
    acc = {}
    for w_id, w in zip(word.tolist(), weight):
        if not w > 0:
            continue
        if w_id not in acc:
            acc[w_id] = np.float32(w)
        elif weighting in (0, 1):
            acc[w_id] = np.float32(acc[w_id] + np.float32(w))
    ids = np.array(sorted(acc), np.uint32)
    vals = np.array([acc[i] for i in ids.tolist()], np.float32)
    nb = len(ids)
    must = scoring != 5
    if weighting in (0, 1) and nb > 0 and not must:
        vals = (vals.astype(np.float64) / float(nb)).astype(np.float32)
    if must:
        norm = 0.0
        if scoring == 1:
            for v in (vals * vals).tolist():  # float32 product, double sum
                norm += v
            norm = float(np.sqrt(np.float64(norm)))
        else:
            for v in vals.tolist():
                norm += abs(v)
        if norm > 0.0:
            vals = (vals.astype(np.float64) / norm).astype(np.float32)
    return ids, vals


def transform(voc, desc, levelsup):
    d = descend(voc, desc, levelsup)
    d["bow_ids"], d["bow_vals"] = assemble(voc, d["word"], d["weight"])
    return d


def _seq_sum(terms):
    t = np.asarray(terms, np.float64)
    return float(np.cumsum(t)[-1]) if len(t) else 0.0


def score(scoring, a, b):
    """score(a, b) of the scoring class `scoring` (0 L1, 1 L2, 2 chi-square, 3 KL, 4 Bhattacharyya, 5 dot); a, b = (ids
    ascending, float32 values)."""
    ai, av = np.asarray(a[0], np.uint32), np.asarray(a[1], np.float32)
    bi, bv = np.asarray(b[0], np.uint32), np.asarray(b[1], np.float32)
    _, ia, ib = np.intersect1d(ai, bi, assume_unique=True, return_indices=True)
    with np.errstate(all="ignore"):
        if scoring == 3:
            terms = np.zeros(len(ai), np.float64)
            use = np.zeros(len(ai), bool)
            matched = np.zeros(len(ai), bool)
            matched[ia] = True
            vi, wi = av[ia], bv[ib]
            both = (vi != 0) & (wi != 0)
            terms[ia] = (vi * np.log(vi / wi)).astype(np.float64)  # float32 throughout
            use[ia] = both
            inside = ~matched & (ai < bi[-1]) if len(bi) else np.zeros(len(ai), bool)  # a larger id of b remains
            tail = ~matched & ~inside
            un = ~matched
            terms[un] = av[un].astype(np.float64) * (np.log(av[un]).astype(np.float64) - LOG_EPS)
            use |= inside | (tail & (av != 0))
            return _seq_sum(terms[use])
        vi, wi = av[ia], bv[ib]
        if scoring == 0:
            s = _seq_sum(np.abs(vi - wi) - np.abs(vi) - np.abs(wi))
            return -s / 2.0
        if scoring in (1, 5):
            s = _seq_sum(vi * wi)
            if scoring == 5:
                return s
            return 1.0 if s >= 1 else float(1.0 - np.sqrt(np.float64(1.0 - s)))
        if scoring == 2:
            keep = (vi + wi) != 0
            return 2.0 * _seq_sum((vi * wi / (vi + wi))[keep])
        if scoring == 4:
            return _seq_sum(np.sqrt(vi * wi))
    raise ValueError(scoring)


def effective(vecs):
    """Padded (ids n x cap, vals n x cap, counts n) -> list of (ids, vals) with min(max(count, 0), cap) entries each."""
    ids, vals, n = vecs
    cap = ids.shape[1]
    return [(ids[i, :min(max(int(c), 0), cap)], vals[i, :min(max(int(c), 0), cap)]) for i, c in enumerate(n)]


def score_all_pairs_symmetric(scoring, q, db):
    """Every query against every database vector for a symmetric scoring, vectorised over the pairs (for the many short
    queries of the launch-loop case): terms in the database vector's id order, one sequential float64 add per slot."""
    assert scoring != 3
    qi, qv, qn = q
    di, dv, dn = db
    cq, cd = qi.shape[1], di.shape[1]
    qok = np.arange(cq)[None, :] < np.clip(qn, 0, cq)[:, None]
    dok = np.arange(cd)[None, :] < np.clip(dn, 0, cd)[:, None]
    acc = np.zeros((len(qi), len(di)), np.float64)
    with np.errstate(all="ignore"):
        for p in range(cd):
            m = (qi[:, None, :] == di[None, :, p, None]) & qok[:, None, :] & dok[None, :, p, None]  # nq x ndb x cq
            found = m.any(axis=2)
            vi = np.where(m, qv[:, None, :], np.float32(0)).sum(axis=2, dtype=np.float32)  # at most one match per row
            wi = np.broadcast_to(dv[None, :, p], vi.shape)
            if scoring == 0:
                term = np.abs(vi - wi) - np.abs(vi) - np.abs(wi)
            elif scoring in (1, 5):
                term = vi * wi
            elif scoring == 2:
                found &= (vi + wi) != 0
                term = vi * wi / (vi + wi)
            else:
                term = np.sqrt(vi * wi)
            acc = np.where(found, acc + term.astype(np.float64), acc)
        if scoring == 0:
            return -acc / 2.0
        if scoring == 1:
            return np.where(acc >= 1, 1.0, 1.0 - np.sqrt(1.0 - np.minimum(acc, 1.0)))
        if scoring == 2:
            return 2.0 * acc
    return acc
