"""Reference for outlier rejection on plane, line, pose prior and relative-pose edge sets (GraphOptimisationOptions::
poseEdgeOutlierRejection; ref: EdgeSet::setOutlierThreshold / updateEdges), numpy only:

    1. the dense LM of relpose_lm_ref.RelPoseGraph for n iterations,
    2. the chi2 term rho(x) of every edge at the final estimates (make_golden.edge, icp_ref.edge_terms,
       prior_ref.edge_terms, relpose_ref.edge_terms),
    3. an edge goes iff its set has a threshold t > 0 and its term is > t,
    4. the LM again on the reduced graph, from those estimates.

Bounds: the rule of icp_lm_ref.tolerances over the reference's own runs (Schur solve against the dense solve, the edges
in another order).  The second run's variants each start from the estimates THEIR first run ended at, so that its
self-sensitivity holds what the first run's round-off does to the second.

Every case is designed so that (a) no term lies within a factor 2 of its threshold on either side — the rejected set
cannot flip by rounding —, (b) the last trial of the first run is accepted — the estimates the optimiser judges at are
the reported ones —, (c) every kind with a threshold loses an edge and keeps one.  reference() asserts all three.

An ICP recipe may hold several sets of a kind (entries of the icp list); thresholds["icp"] has one value per entry.
"""
import numpy as np

import icp_lm_ref
import icp_ref
import prior_ref as PR
import relpose_lm_ref as L
import relpose_ref as RR

import make_golden as mg  # (icp_lm_ref put tests/golden on the path)

KINDS = ("plane", "line", "prior", "relpose")  # the kind codes 0 .. 3 of cugo_graph_n_pose_edge_outliers


def bump(pose7, rot, trans):
    return icp_ref.left_update(pose7, np.concatenate([np.asarray(rot, float), np.asarray(trans, float)]))


# ---- the cases -------------------------------------------------------------------------------------------------
def closure_graph(seed, false_edges, closures, closure_scale=2.0, rk=(RR.RK_HUBER, 3.0)):
    """8 poses, no landmarks, pose 0 fixed; 7 odometry edges in alternating orientation, the first with its fixed end;
    `closures` on top; the edges listed in false_edges get a measurement displaced by ~1 rad and several units"""
    rng = np.random.default_rng(seed)
    P = 8
    gt = np.array([icp_ref.random_pose(rng, rot=0.4) for _ in range(P)])
    pose = gt.copy()
    for i in range(1, P):
        pose[i] = PR.displaced(rng, gt[i], 0.1, 0.5)
    pf = np.zeros(P, np.uint8)
    pf[0] = 1
    odo = L.edges_between(rng, gt, [(i, i + 1) if i % 2 == 0 else (i + 1, i) for i in range(P - 1)], 0.01, 0.05, 50.0)
    clo = L.edges_between(rng, gt, closures, 0.01, 0.05, closure_scale)
    rp = RR.make_edges(np.concatenate([odo["a"], clo["a"]]), np.concatenate([odo["b"], clo["b"]]),
                       np.concatenate([odo["z"], clo["z"]]), np.concatenate([odo["info"], clo["info"]]), rk=rk)
    for e in false_edges:
        rp["z"][e] = bump(rp["z"][e], [0.6, -0.5, 0.6], [3.0, -2.5, 3.5])
    return L.no_ba(pose, pf, gt), [], L.empty_prior(), rp


def closures_case():
    """closures 7: (1, 5) true, 8: (5, 1) FALSE on the pair of 7, 9: (2, 7) FALSE and alone on its pair"""
    d, icp, prior, rp = closure_graph(21, false_edges=(8, 9), closures=[(1, 5), (5, 1), (2, 7)])
    return d, icp, prior, rp, dict(relpose=35.0)


def closures_fixed_end_case():
    """the false closure is the one with a fixed end, (4, 0): only the diagonal term of pose 4 and its b go with it (the
    odometry edge (0, 1) keeps the gauge)"""
    d, icp, prior, rp = closure_graph(22, false_edges=(8,), closures=[(1, 5), (4, 0), (2, 7)])
    return d, icp, prior, rp, dict(relpose=35.0)


def icp_case():
    """icp_lm_ref.icp_only_case with gross outliers planted: the plane edges in TWO sets — the first 200 with a threshold,
    the other 85 with threshold 0, gross outliers in both (those of the second set stay) — and the line set with its own"""
    d, icp = icp_lm_ref.icp_only_case()
    (_, pl, om_pl, act_pl, rk_pl), (_, li, om_li, act_li, rk_li) = icp
    pl = {k: v.copy() for k, v in pl.items()}
    li = {k: v.copy() for k, v in li.items()}
    free = np.flatnonzero(pl["pose"] != 5)
    for e in list(free[[3, 50, 111]]) + list(free[free >= 200][[2, 30]]):
        pl["d"][e] += 6.0
    lfree = np.flatnonzero(li["pose"] != 5)
    for e in lfree[[1, 20]]:
        off = np.array([4.0, -5.0, 4.5])
        li["a"][e] += off
        li["b"][e] += off
    A = {k: v[:200] for k, v in pl.items()}
    B = {k: v[200:] for k, v in pl.items()}
    icp = [("plane", A, om_pl, act_pl[:200], rk_pl), ("plane", B, om_pl, act_pl[200:], rk_pl),
           ("line", li, om_li, act_li, rk_li)]
    return d, icp, L.empty_prior(), None, dict(icp=[5.0, 0.0, 1.5])


def gps_case():
    """prior_ref.corridor_case (planes that leave x unobserved + one weak prior per free pose): the prior of pose 2 is false"""
    d, icp, prior = PR.corridor_case()
    prior = dict(prior, z=prior["z"].copy())
    prior["z"][2] = bump(prior["z"][2], [0.7, 0.5, -0.6], [4.0, 3.0, -3.5])
    return d, icp, prior, None, dict(prior=1.0)


def mixed_case():
    """relpose_lm_ref.mixed_case with gross outliers in every set: mono and stereo BA edges 40 px off, planes, lines, a
    false prior on pose 3 next to a true one, a false second edge on an odometry pair; thresholds on all six sets"""
    d, icp, prior, rp = L.mixed_case()
    d = dict(d, e_meas=np.asarray(d["e_meas"], np.float64).copy())
    st = np.asarray(d["e_stereo"]).astype(bool)
    for e in list(np.flatnonzero(~st)[[1, 7]]) + list(np.flatnonzero(st)[[2, 11, 23]]):
        d["e_meas"][e, :2] += np.array([40.0, -35.0])
    (_, pl, om_pl, act_pl, rk_pl), (_, li, om_li, act_li, rk_li) = icp
    pl = {k: v.copy() for k, v in pl.items()}
    li = {k: v.copy() for k, v in li.items()}
    for e in np.flatnonzero(pl["pose"] != 0)[[0, 9]]:
        pl["d"][e] += 0.8
    for e in np.flatnonzero(li["pose"] != 0)[[1, 6]]:
        li["a"][e] += np.array([0.6, -0.7, 0.5])
        li["b"][e] += np.array([0.6, -0.7, 0.5])
    icp = [("plane", pl, om_pl, act_pl, rk_pl), ("line", li, om_li, act_li, rk_li)]
    rng = np.random.default_rng(5)
    gt = d["pose_gt"]
    prior = PR.make_prior([3, 5, 3], list(prior["z"]) + [bump(gt[3], [0.3, -0.3, 0.25], [0.6, 0.5, -0.6])],
                          list(prior["info"]) + [PR.random_spd(rng, 50.0)], rk=prior["rk"])
    rp = dict(rp, z=rp["z"].copy())
    rp["z"][5] = bump(rp["z"][5], [0.3, 0.25, -0.3], [0.6, -0.5, 0.6])  # (3, 2): the second edge of its pair
    return d, icp, prior, rp, dict(ba=(55.0, 30.0), ba_rk=(3, 3.0), icp=[70.0, 150.0], prior=40.0, relpose=60.0)


# name -> (recipe, iterations of the first optimize(), of the second).  Without its outliers a graph is nearly converged
# where the first run ended: the second run is kept as short as its steps still gain (|rho| >= 0.1 is asserted)
CASES = {
    "closures": (closures_case, 6, 3),
    "closures_fixed_end": (closures_fixed_end_case, 6, 2),
    "icp": (icp_case, 4, 2),
    "gps": (gps_case, 4, 1),
    "mixed": (mixed_case, 8, 8),
}


# ---- the reference -----------------------------------------------------------------------------------------------
def no_relpose():
    return RR.make_edges([], [], np.zeros((0, 7)), np.eye(6)[None])


def lm_runs(d, icp, prior, rp, niter, starts=None, rk=(0, 1.0)):
    """relpose_lm_ref.reference_runs that also hands out every variant's final estimates, and can start every variant
    from estimates of its own.  -> (trace dicts, pose, lm, chi2 self-sensitivity per iteration, that of the estimates,
    [(pose, lm) per variant])"""
    rp = no_relpose() if rp is None else rp
    runs = []
    variants = ((icp, prior, rp, True), (icp, prior, rp, False),
                (icp_lm_ref.permuted(icp), PR.permuted_prior(prior), L.permuted_relpose(rp), True))
    for k, (icp_k, pr_k, rp_k, vs) in enumerate(variants):
        dk = d if starts is None else dict(d, pose=starts[k][0], lm=starts[k][1])
        g = L.RelPoseGraph(dk, icp_k, pr_k, rp_k, rk, via_schur=vs)
        runs.append((g.optimize(niter), g.pose.copy(), g.lm.copy()))
    tr = runs[0][0]
    sens, est = [0.0] * len(tr), 0.0
    for t2, pose2, lm2 in runs[1:]:
        assert [t[4] for t in t2] == [t[4] for t in tr], "the reference disagrees with itself on the trial counts"
        for i in range(len(tr)):
            sens[i] = max(sens[i], abs(tr[i][1] - t2[i][1]) / abs(tr[i][1]))
        est = max(est, float(np.abs(runs[0][1] - pose2).max()), float(np.abs(runs[0][2] - lm2).max()) if len(lm2) else 0.0)
    return icp_lm_ref.trace_dicts(tr), runs[0][1], runs[0][2], sens, est, [(r[1], r[2]) for r in runs]


def edge_terms(d, icp, prior, rp, pose, lm, rk=(0, 1.0)):
    """the chi2 term of every edge at (pose, lm), NaN for an edge that does not count (inactive, on fixed vertices only):
    dict ba [E], icp [per entry [E]], prior [E], relpose [E]"""
    pf = np.asarray(d["pose_fixed"]).astype(bool)
    lf = np.asarray(d["lm_fixed"]).astype(bool)
    out = dict(ba=np.full(len(d["e_pose"]), np.nan), icp=[], prior=np.full(len(prior["pose"]), np.nan),
               relpose=np.full(0 if rp is None else len(rp["a"]), np.nan))
    for k in range(len(d["e_pose"])):
        ip, il = d["e_pose"][k], d["e_lm"][k]
        if not (pf[ip] and lf[il]):
            e = mg.edge(pose[ip], lm[il], d["e_meas"][k], bool(d["e_stereo"][k]), d["e_cam"][k])[0]
            out["ba"][k] = mg.rho(rk[0], rk[1], d["e_omega"][k] * (e @ e))
    for kind, e, om, act, rk in icp:
        om = np.broadcast_to(np.asarray(om, np.float64), (len(act),))
        t = np.full(len(act), np.nan)
        for i in range(len(act)):
            if act[i] and not pf[e["pose"][i]]:
                t[i] = icp_ref.edge_terms(kind, e, i, pose[e["pose"][i]], om[i], rk)[0]
        out["icp"].append(t)
    info = np.broadcast_to(prior["info"], (len(prior["pose"]), 6, 6))
    for i, p in enumerate(prior["pose"]):
        if prior["active"][i] and not pf[p]:
            out["prior"][i] = PR.edge_terms(pose[p], prior["z"][i], info[i], prior.get("rk", (0, 1.0)))[0]
    if rp is not None:
        info = np.broadcast_to(rp["info"], (len(rp["a"]), 6, 6))
        for i, (a, b) in enumerate(zip(rp["a"], rp["b"])):
            if rp["active"][i] and not (pf[a] and pf[b]):
                out["relpose"][i] = RR.edge_terms(pose[a], pose[b], rp["z"][i], info[i], rp.get("rk", (0, 1.0)))[0]
    return out


def thresholds_per_edge(d, icp, prior, rp, thr):
    """the threshold of every edge's set, laid out as edge_terms lays out the terms"""
    st = np.asarray(d["e_stereo"]).astype(bool)
    ba = thr.get("ba", (0.0, 0.0))
    return dict(ba=np.where(st, ba[1], ba[0]).astype(float),
                icp=[np.full(len(e[3]), t) for e, t in zip(icp, thr.get("icp", [0.0] * len(icp)))],
                prior=np.full(len(prior["pose"]), thr.get("prior", 0.0)),
                relpose=np.full(0 if rp is None else len(rp["a"]), thr.get("relpose", 0.0)))


def flat(x):
    return np.concatenate([np.ravel(v) for v in (x["ba"], *x["icp"], x["prior"], x["relpose"])])


def rejected_sets(terms, thr_e):
    """boolean masks in the layout of edge_terms (a NaN term compares false: kept)"""
    with np.errstate(invalid="ignore"):
        rej = lambda t, th: (th > 0) & (t > th)
        return dict(ba=rej(terms["ba"], thr_e["ba"]), icp=[rej(t, th) for t, th in zip(terms["icp"], thr_e["icp"])],
                    prior=rej(terms["prior"], thr_e["prior"]), relpose=rej(terms["relpose"], thr_e["relpose"]))


def reduced(d, icp, prior, rp, rej, pose, lm):
    """the graph without the rejected edges, at the given estimates"""
    keep = ~rej["ba"]
    d2 = dict(d, pose=pose, lm=lm)
    for k in ("e_pose", "e_lm", "e_stereo", "e_meas", "e_omega", "e_cam"):
        d2[k] = np.asarray(d[k])[keep]
    icp2 = [(kind, e, om, np.asarray(act, bool) & ~r, rk) for (kind, e, om, act, rk), r in zip(icp, rej["icp"])]
    prior2 = dict(prior, active=np.asarray(prior["active"], bool) & ~rej["prior"])
    rp2 = None if rp is None else dict(rp, active=np.asarray(rp["active"], bool) & ~rej["relpose"])
    return d2, icp2, prior2, rp2


_REF = {}


def reference(name):
    """dict of a case: the recipe (d, icp, prior, rp, thr, niter, niter2), the first run (tr, pose, lm, tol, etol), the terms at
    its end and the rejected sets (terms, rej), the reduced graph (d2, icp2, prior2, rp2) and the run on it (tr2, pose2,
    lm2, tol2, etol2); the design conditions (a) - (c) asserted on the way"""
    if name in _REF:
        return _REF[name]
    recipe, niter, niter2 = CASES[name]
    d, icp, prior, rp, thr = recipe()
    rk = thr.get("ba_rk", (0, 1.0))  # the robust kernel of the mono and stereo sets
    tr, pose, lm, sens, est, ends = lm_runs(d, icp, prior, rp, niter, rk=rk)
    assert len(tr) == niter, (name, len(tr))
    assert all(abs(t["rho"]) >= 0.1 for t in tr), "a decision at rho near 0 is not a fair comparison"
    assert tr[-1]["rho"] > 0, "(b) the last trial of the first run must be an accepted one"
    terms = edge_terms(d, icp, prior, rp, pose, lm, rk)
    thr_e = thresholds_per_edge(d, icp, prior, rp, thr)
    t, th = flat(terms), flat(thr_e)
    judged = (th > 0) & ~np.isnan(t)
    near = judged & (t > 0.5 * th) & (t < 2.0 * th)
    assert not near.any(), "(a) a term within a factor 2 of its threshold: %s against %s" % (t[near], th[near])
    rej = rejected_sets(terms, thr_e)
    for e_ends in ends[1:]:  # the variants reject the same edges: the sets are the reference's
        tv = edge_terms(d, icp, prior, rp, e_ends[0], e_ends[1], rk)
        assert np.array_equal(flat(rejected_sets(tv, thr_e)), flat(rej))
    st = np.asarray(d["e_stereo"]).astype(bool)
    sets = [("mono", terms["ba"][~st], thr_e["ba"][~st], rej["ba"][~st]), ("stereo", terms["ba"][st], thr_e["ba"][st], rej["ba"][st]),
            ("prior", terms["prior"], thr_e["prior"], rej["prior"]), ("relative-pose", terms["relpose"], thr_e["relpose"], rej["relpose"])]
    sets += [("%s set %d" % (e[0], i), terms["icp"][i], thr_e["icp"][i], rej["icp"][i]) for i, e in enumerate(icp)]
    for what, t_s, th_s, r_s in sets:
        on = (th_s > 0) & ~np.isnan(t_s)
        if on.any():
            assert (r_s & on).any() and (~r_s & on).any(), "(c) the %s set must lose an edge and keep one" % what
        else:
            assert not r_s.any()
    d2, icp2, prior2, rp2 = reduced(d, icp, prior, rp, rej, pose, lm)
    tr2, pose2, lm2, sens2, est2, _ = lm_runs(d2, icp2, prior2, rp2, niter2, starts=ends, rk=rk)
    assert len(tr2) == niter2 and all(abs(t["rho"]) >= 0.1 for t in tr2), "a decision at rho near 0 is not a fair comparison (second run)"
    tol, etol = icp_lm_ref.tolerances(sens, est)
    tol2, etol2 = icp_lm_ref.tolerances(sens2, est2)
    print("reference %s: self-sensitivity %.3g / %.3g (chi2), %.3g / %.3g (estimates); rejected %d of %d judged edges" %
          (name, max(sens), max(sens2), est, est2, int(flat(rej).sum()), int(judged.sum())))
    _REF[name] = dict(rk=rk, d=d, icp=icp, prior=prior, rp=rp, thr=thr, niter=niter, niter2=niter2, tr=tr, pose=pose, lm=lm, tol=tol, etol=etol,
                      terms=terms, rej=rej, d2=d2, icp2=icp2, prior2=prior2, rp2=rp2, tr2=tr2, pose2=pose2, lm2=lm2,
                      tol2=tol2, etol2=etol2)
    return _REF[name]


# ---- the product's graph from a recipe ---------------------------------------------------------------------------
def product_index(active, mask):
    """positions, among the edges the C graph object holds (the active ones, in order), of the edges in `mask`"""
    return np.flatnonzero(np.asarray(mask)[np.asarray(active, bool)])


def set_thresholds(g, cugo, thr, scale=1.0):
    """the case's thresholds (times scale) on the sets of a cugo Graph: one plane set, one line set (an ICP recipe with
    several sets of a kind does not fit the C graph object)"""
    ba = thr.get("ba", (0.0, 0.0))
    g.set_outlier_threshold(2, ba[0] * scale)
    g.set_outlier_threshold(3, ba[1] * scale)
    icp = thr.get("icp", [])
    assert len(icp) in (0, 2)
    if icp:
        g.set_icp_outlier_threshold(cugo.ICP_PLANE, icp[0] * scale)
        g.set_icp_outlier_threshold(cugo.ICP_LINE, icp[1] * scale)
    g.set_prior_outlier_threshold(thr.get("prior", 0.0) * scale)
    g.set_relpose_outlier_threshold(thr.get("relpose", 0.0) * scale)


def build_graph(cugo, r, thr="case", plan_only=False, option=True, scale=1.0):
    """the cugo Graph of a reference() dict: thr "case" = the case's thresholds, a dict of that form, or None for none"""
    thr = r["thr"] if isinstance(thr, str) else thr
    g = L.build_graph(r["d"], r["icp"], r["prior"], r["rp"], rk=r["rk"], plan_only=plan_only)
    if option:
        g.set_option("pose_edge_outliers", 1)
    if thr is not None:
        set_thresholds(g, cugo, thr, scale)
    return g
