"""The exact restatement of the evaluation kernels (tests/eval_restate.py, second half) on the host: it agrees with the torch
form on the golden fixture and on hand-built rows (ties, NaN, every bin edge), its checks reject realistic corruptions of a
correct table, and the evaluator refuses labels its kernels would drop."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import eval_restate as R  # noqa: E402
from test_eval_cpu import GOLD, NS, gt_of, restated_tables  # noqa: E402

NAN, INF = float("nan"), float("inf")
SUB = float(np.float32(1e-45))               # smallest fp32 subnormal


def argmax_rows_cases():
    return np.array([
        [0.5, 0.5, 0.1, 0.1],                # tie at index 0
        [0.1, 0.7, 0.2, 0.7],                # tie in the middle
        [0.25, 0.25, 0.25, 0.25],            # all equal
        [-0.0, 0.0, -0.0, 0.0],              # -0.0 == +0.0: index 0
        [0.0, -0.0, 0.0, 0.0],
        [SUB, 2 * SUB, 0.0, 2 * SUB],        # subnormals
        [NAN, 0.9, 0.1, 0.0],                # NaN first
        [0.1, NAN, 0.5, 0.4],                # NaN later
        [0.1, 0.2, NAN, NAN],                # two NaNs: the first
        [INF, 0.2, NAN, 1.0],                # NaN beats +inf
        [-INF, -INF, -INF, -INF],
        [0.0, 0.0, 0.0, 1.0],
    ], np.float32)


def edge_confidences():
    """Every fp32 edge of torch.linspace(0, 1, 16) with its nextafter neighbours, and the values outside [0, 1]."""
    e = R.EDGES.numpy()
    v = np.concatenate([e, np.nextafter(e, np.float32(-1)), np.nextafter(e, np.float32(2))])
    return np.concatenate([v, np.array([0.0, -0.0, -0.25, 1.0, 1.5, 600.0, -700.0, INF, -INF, NAN, SUB], np.float32)])


def test_argmax_restatement_is_torch_argmax():
    p = argmax_rows_cases()
    assert np.array_equal(R.argmax_rows(p), torch.from_numpy(p).argmax(1).numpy())
    assert R.argmax_rows(p)[[6, 7, 8, 9]].tolist() == [0, 1, 2, 2]
    g = np.random.default_rng(0)
    q = g.integers(0, 4, (2000, 7)).astype(np.float32) / 4          # many ties
    q[g.random(q.shape) < 0.02] = np.nan
    assert np.array_equal(R.argmax_rows(q), torch.from_numpy(q).argmax(1).numpy())


def test_bin_restatement_is_torch_bucketize_at_every_edge():
    c = edge_confidences()
    got = R.bin_index(c)
    assert np.array_equal(got, R.bins_of(torch.from_numpy(c)).numpy())
    e = R.EDGES.numpy()
    assert np.array_equal(got[:16], np.arange(16))                            # an edge opens its bin
    assert np.array_equal(got[17:32], np.arange(15))                          # one ulp below closes the previous
    assert got[16] == 0 and got[-2] == 15 and R.bin_index(np.float32([NAN]))[0] == 15
    assert R.bin_index(np.float32([-0.25, -INF]))[0] == 0
    assert e[-1] == 1.0 and R.bin_index(np.float32([1.0]))[0] == 15


def test_fixed_point_terms():
    c = np.float32([1.0, 0.5, -0.25, NAN, INF, -INF, 600.0, -700.0, 2.0 ** -38, 3 * 2.0 ** -37])
    fx = R.conf_fixed(c)
    assert fx.tolist() == [2 ** 36, 2 ** 35, -2 ** 34, 0, 0, 0, 512 * 2 ** 36, -512 * 2 ** 36, 0, 2]   # half to even
    big = np.full(5, 2 ** 45, np.int64)
    assert R.keyed_sum(np.zeros(5, np.int64), big, 1) == [5 * 2 ** 45]
    assert R.keyed_sum(np.array([0, 1, 1]), np.array([-3, 2 ** 62, 2 ** 62]), 2) == [-3, 2 ** 63]
    assert R.fx_value(2 ** 63, 36) == 2.0 ** 27
    t = R.nll_terms(np.float32([1.0, 0.0, -1.0, INF]))
    assert t[1] == np.float32(-np.log(np.float32(1e-12))) and np.isnan(t[2]) and t[3] == -INF
    assert R.nll_fixed(t)[2:].tolist() == [0, 0]


def test_exact_restatement_agrees_with_the_torch_form_on_the_fixture():
    for k in range(NS):
        gt = gt_of(k)
        for o, exp in enumerate(restated_tables(k, gt)):
            ex = exp["exact"]
            for key in ("cm", "bin_count", "bin_correct"):
                assert np.array_equal(ex[key], exp[key]), (k, o, key)
            assert ex["unknown"] == exp["unknown"]
            # the torch form sums in fp64: within the fixed-point format's cost of it
            fx = np.array([R.fx_value(v, R.CONF_SHIFT) for v in ex["bin_conf_fx"].reshape(-1)]).reshape(2, -1)
            assert (np.abs(fx - exp["bin_conf"]) <= ex["bin_count"] * 2.0 ** -37 + 1e-12).all()
            nll = np.array([R.fx_value(v, R.NLL_SHIFT) for v in ex["nll_fx"]])
            assert (np.abs(nll - exp["nll"]) <= ex["nll_n"] * 2.0 ** -31 + ex["nll_ulp"]).all()   # torch's log, numpy's log
            # the restatement's own table passes its own check
            got = dict(exp, bin_conf=fx, nll=nll)
            R.check_ssc(got, ex)
            R.check_conf_sums([R.fx_value(v, R.CONF_SHIFT) for v in exp["mask_conf_fx"]], exp["mask_conf_fx"],
                              exp["mask_conf_fp64"], exp["mask_count"], "mask_conf")


def test_row_restatement_agrees_with_the_dense_form_on_the_fixture():
    for k in range(NS):
        gt = gt_of(k)
        for o, exp in enumerate(restated_tables(k, gt)):
            pan = GOLD["in_pan"][k, o].astype(np.int64)
            vconf = GOLD["in_vconf"][k, o].astype(np.float32)
            site = np.flatnonzero((pan != 0) | (vconf != 0))
            P = exp["area"].shape[0] - 1
            ex = R.rows_exact(site, pan[site], vconf[site], GOLD["in_sem"][k], gt.panoptic.numpy(), gt.gt_area.numpy(), P,
                              gt.n_gt)
            assert np.array_equal(ex["area"][1:], exp["area"][1:]) and np.array_equal(ex["inter"][:, 1:], exp["inter"][:, 1:])
            for key in ("map", "mask_count", "mask_correct", "mask_conf_fx"):
                assert np.array_equal(np.asarray(ex[key]), np.asarray(exp[key])), (k, o, key)


def _case(n=4000, seed=1, C=5):
    g = np.random.default_rng(seed)
    probs = g.dirichlet(np.ones(C), n).astype(np.float32)
    probs[g.random(n) < 0.3, 0] = 0.95                            # a populated pred == 0 group
    conf = probs.max(1).astype(np.float32)
    conf[:40] = R.EDGES.numpy()[g.integers(0, 16, 40)]             # sites exactly at edges
    conf[40:44] = 3e-4                                             # a few in the low bin
    sem = g.integers(0, C, n).astype(np.uint8)
    sem[g.random(n) < 0.05] = 255
    return probs, conf, sem


def _table_of(ex, nll=None):
    """The table a correct kernel returns for `ssc_exact` tables `ex`."""
    return {"cm": ex["cm"], "unknown": ex["unknown"], "bin_count": ex["bin_count"].copy(),
            "bin_correct": ex["bin_correct"].copy(),
            "bin_conf": np.array([R.fx_value(v, R.CONF_SHIFT) for v in ex["bin_conf_fx"].reshape(-1)]).reshape(2, -1),
            "nll": np.array([R.fx_value(v, R.NLL_SHIFT) for v in ex["nll_fx"]]) if nll is None else nll}


def _old_check(got, exp):
    """The tolerance tests/test_hip_eval.py used before: atol = 1e-6 * max |whole array|."""
    for key in ("bin_conf", "nll"):
        np.testing.assert_allclose(got[key], exp[key], rtol=1e-6, atol=1e-6 * max(1.0, float(np.abs(exp[key]).max())))


def _run_cached_bins(keys, conf, off_by_one):
    """The kernels' run caching over one thread's sites; `off_by_one` flushes the first site of a new run with the old key."""
    cnt, fx = np.zeros(2 * R.BINS, np.int64), [0] * (2 * R.BINS)
    key, n, s = -1, 0, 0
    vals = R.conf_fixed(conf)
    for k, v in zip(keys.tolist(), vals.tolist()):
        if k != key:
            if key >= 0:
                if off_by_one:
                    n, s = n + 1, s + v
                cnt[key] += n
                fx[key] += s
            key, n, s = k, (-1 if off_by_one else 0), (-v if off_by_one else 0)
        n, s = n + 1, s + v
    cnt[key] += n
    fx[key] += s
    return cnt, fx


def test_checks_reject_realistic_corruptions():
    probs, conf, sem = _case()
    ex = R.ssc_exact(probs, conf, sem)
    R.check_ssc(_table_of(ex), ex)
    known = sem != 255
    pred = R.argmax_rows(probs[known])
    grp = (pred != 0).astype(np.int64)

    # 1. one site moved to the neighbouring bin: a conf exactly at an edge taken one ulp below it
    c2 = conf.copy()
    i = next(j for j in range(40) if known[j] and conf[j] > 0)
    c2[i] = np.nextafter(conf[i], np.float32(0))
    with pytest.raises(AssertionError, match="bin_count"):
        R.check_ssc(_table_of(R.ssc_exact(probs, c2, sem)), ex)

    # 2. one site's confidence dropped from a small bin: the counts hold, the old tolerance passed it
    t = _table_of(ex)
    key = grp * R.BINS + R.bin_index(conf[known])
    j = int(np.flatnonzero(conf[known] == np.float32(3e-4))[0])
    assert R.bin_index(conf[known][j:j + 1])[0] == 0
    t["bin_conf"][grp[j], 0] -= float(conf[known][j])
    _old_check(t, _table_of(ex))
    with pytest.raises(AssertionError, match="bin_conf"):
        R.check_ssc(t, ex)

    # 3. the groups swapped
    t = _table_of(ex)
    for k in ("bin_count", "bin_correct", "bin_conf", "nll"):
        t[k] = t[k][::-1].copy()
    with pytest.raises(AssertionError):
        R.check_ssc(t, ex)
    t = _table_of(ex)
    t["nll"] = t["nll"][::-1].copy()                                  # the -log sums alone
    with pytest.raises(AssertionError, match="nll"):
        R.check_ssc(t, ex)

    # 4. an off-by-one flush of a run: counts and sums from a run cache that hands a site to the previous key
    keys = key
    good_cnt, good_fx = _run_cached_bins(keys, conf[known], False)
    assert np.array_equal(good_cnt, ex["bin_count"].reshape(-1)) and good_fx == list(ex["bin_conf_fx"].reshape(-1))
    bad_cnt, bad_fx = _run_cached_bins(keys, conf[known], True)
    t = _table_of(ex)
    t["bin_conf"] = np.array([R.fx_value(v, R.CONF_SHIFT) for v in bad_fx]).reshape(2, -1)
    with pytest.raises(AssertionError, match="bin_conf"):
        R.check_ssc(t, ex)                                          # even with the counts left right
    t["bin_count"] = bad_cnt.reshape(2, -1)
    with pytest.raises(AssertionError, match="bin_count"):
        R.check_ssc(t, ex)

    # 5. -log summed in fp32 (sequentially, as float atomics would) instead of fixed point
    g = sem[known].astype(np.int64)
    terms = R.nll_terms(probs[known][np.arange(g.shape[0]), g])
    nll32 = np.array([float(np.cumsum(terms[grp == k], dtype=np.float32)[-1]) for k in range(2)])
    with pytest.raises(AssertionError, match="nll"):
        R.check_ssc(_table_of(ex, nll=nll32), ex)


def test_mask_checks_reject_a_dropped_site():
    g = np.random.default_rng(5)
    n, S = 3000, 5000
    site = g.integers(-2, S + 2, n)
    pred = g.integers(-1, 9, n).astype(np.int64)
    conf = g.random(n).astype(np.float32)
    sem = np.where(g.random(S) < 0.1, 255, 1).astype(np.uint8)
    gt_id = g.integers(0, 6, S)
    gt_area = np.bincount(gt_id, minlength=6) + 3
    ex = R.rows_exact(site, pred, conf, sem, gt_id, gt_area, 8, 5)
    vals = np.array([R.fx_value(v, R.CONF_SHIFT) for v in ex["mask_conf_fx"]])
    R.check_conf_sums(vals, ex["mask_conf_fx"], ex["mask_conf_fp64"], ex["mask_count"], "mask_conf")
    b = int(np.argmax(ex["mask_count"]))
    vals[b] = np.nextafter(vals[b], 0)                               # one ulp of the whole bin
    with pytest.raises(AssertionError, match="mask_conf"):
        R.check_conf_sums(vals, ex["mask_conf_fx"], ex["mask_conf_fp64"], ex["mask_count"], "mask_conf")


def test_nll_bound_is_the_rounding_plus_nll_ulps_per_term():
    probs, conf, sem = _case(n=500, seed=2)
    ex = R.ssc_exact(probs, conf, sem)
    t = _table_of(ex)
    edge = ex["nll_n"] * 2.0 ** -30 + R.NLL_ULPS * ex["nll_ulp"]
    R.check_ssc(dict(t, nll=t["nll"] + 0.99 * edge), ex)
    with pytest.raises(AssertionError, match="nll"):
        R.check_ssc(dict(t, nll=t["nll"] + edge + 0.5 * ex["nll_ulp"]), ex)


def test_evaluator_refuses_labels_beyond_its_classes():
    """A 20-class label grid scored at 19 classes: pe_ssc would drop every site labelled 19 without a word."""
    from pasco_amd.eval import GroundTruth, SceneEvaluator
    sem = np.zeros((4, 4, 2), np.uint8)
    sem[0, 0, 0], sem[1, 1, 1] = 19, 255
    gt = GroundTruth.from_labels(sem, np.zeros_like(sem), (1,))
    assert gt.max_label == 19 and gt.to("cpu").max_label == 19
    ev = SceneEvaluator(n_classes=19, thing_ids=(1, 2, 3, 4, 5, 6), n_outputs=1)
    with pytest.raises(ValueError, match="label 19"):
        ev.add_tables([{}], gt)
    with pytest.raises(ValueError, match="label 19"):
        ev.add([None], [torch.zeros(19, 4, 4, 2)], gt)
    sem[0, 0, 0] = 18                                                # 18 and unknown (255) are in range
    assert GroundTruth.from_labels(sem, np.zeros_like(sem), (1,)).max_label == 18
    assert GroundTruth.from_labels(np.full((2, 2, 2), 255, np.uint8), np.zeros((2, 2, 2), np.uint8), (1,)).max_label == -1
