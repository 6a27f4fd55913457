"""The routing of the fused MLP chain and of the single fused layer as plain data (no GPU): fused._plan_chain against the
launches recorded for the BASELINE step, the couplings between its forward and backward parts over a sweep of shapes and
switches, and fused._layer_route against the conditions of each of its five paths."""
import contextlib
import itertools

from torch_points3d_amd import _lib, fused
from test_plans_cpu import CHANNELS, ROWS


@contextlib.contextmanager
def _switch(name, value):
    keep = getattr(fused, name)
    setattr(fused, name, value)
    try:
        yield
    finally:
        setattr(fused, name, keep)


def _fwd(plan):
    return [(p.kernel, p.chunks, p.reverse, p.keep_act) for p in plan]


def _bwd(plan):
    """last layer to first: (reductions: own pass direction / None = from the layer above), (input-gradient kind, columns,
    direction, dY written), (weight-gradient kernel, chunks, direction)"""
    return [(p.bwd.reduce_rev, (p.bwd.kind, p.bwd.cols, p.bwd.dx_rev, p.bwd.write_dY), (p.bwd.wgrad, p.bwd.wgrad_chunks, p.bwd.wgrad_rev))
            for p in reversed(plan)]


# the three chains of the BASELINE step (unet_3_ss, B=32, N=16384): M, K0, widths, pool, input gradient wanted, grad_cols
DOWN0 = (1048576, 8, [64, 64, 128], 64, False, (3, 3))
DOWN1 = (262144, 132, [128, 128, 256], 64, True, (3, 128))
UP2 = (524288, 132, [128, 128, 128], 0, True, (0, 128))


def _baseline_plan(chain):
    M, K0, widths, pool, need_in, cols = chain
    return fused._plan_chain(M, K0, widths, pool, True, need_in, [True] * len(widths), cols)


def test_baseline_step_plans():
    """the launches of the training step at the BASELINE size, as recorded from the decision code before it became a plan"""
    red = ("x3_act_red", 256, 1)
    plan = _baseline_plan(DOWN0)
    assert _fwd(plan) == [("narrow", 1024, 1, False), ("sp", 1024, 0, False), ("x3", 1024, 1, False)]
    assert _bwd(plan) == [(1, ("loader", None, 0, True), red), (None, ("loader", None, 0, True), red),
                          (None, ("narrow", None, None, False), ("narrow", 0, 0))]
    plan = _baseline_plan(DOWN1)
    assert _fwd(plan) == [("x3_identity", 1024, 1, False), ("x3", 1024, 0, False), ("x3", 512, 1, False)]
    assert _bwd(plan) == [(1, ("loader", None, 0, True), red), (None, ("loader", None, 0, True), red),
                          (None, ("loader", (3, 128), 0, True), ("x3", 0, 1))]
    plan = _baseline_plan(UP2)
    assert _fwd(plan) == [("x3_identity", 1024, 1, False), ("x3", 1024, 0, False), ("x3", 1024, 1, False)]
    assert _bwd(plan) == [(1, ("loader", None, 0, True), red), (None, ("loader", None, 0, True), red),
                          (None, ("loader", (0, 128), 0, True), ("x3", 0, 1))]
    assert all(p.bwd.terms == 6 for p in plan)


def test_nine_term_plan_keeps_the_skipped_turn():
    """WGRAD_X3 = 9: the kernel that also reduces declines, its turn is still taken, so the weight-gradient kernel that
    runs instead walks front to back"""
    with _switch("WGRAD_X3", 9):
        plan = _baseline_plan(UP2)
    act = ("x3_act", 0, 0)
    assert _bwd(plan) == [(1, ("loader", None, 0, True), act), (1, ("loader", None, 0, True), act),
                          (1, ("loader", (0, 128), 0, True), ("x3", 0, 1))]
    assert all(p.bwd.terms == 9 for p in plan)


CHAIN_SWITCHES = [("FWD_X3", False), ("WGRAD_X3_ACT", False), ("WGRAD_X3", 0), ("WGRAD_X3", 9), ("CHAIN_BWD_LOADER", False),
                  ("CHAIN_BWD_POOLED", False), ("ROW_ORDER_ALTERNATE", False), ("WGRAD_NARROW", False), ("FWD_NARROW", False),
                  ("WGRAD_RED", False)]
WIDTHS = [[64, 128], [128, 128], [32, 64], [128, 196], [256, 132], [64, 64, 128], [128, 128, 256], [128, 128, 128],
          [64, 96, 128], [32, 64, 1024], [516, 256, 1536], [128, 260, 128]]


def _check_couplings(M, K0, widths, pool, need_in, need_w, cols, plan):
    h = _lib.load()
    L = len(widths)
    Ks = [K0] + widths[:-1]
    assert len(plan) == L and not plan[0].keep_act
    for l, p in enumerate(plan):
        N, K, b, ctx = widths[l], Ks[l], p.bwd, (M, K0, widths, pool, need_in, need_w, cols, l)
        side = int(p.keep_act)
        want = {"x3_identity": h.tp3d_gemm_rows_x3_chunks(M, N, K, 0), "x3": h.tp3d_gemm_rows_x3_chunks(M, N, K, side),
                "sp": h.tp3d_gemm_rows_sp_chunks(M, N, K, side), "narrow": h.tp3d_gemm_rows_narrow_chunks(M),
                "rows": h.tp3d_gemm_rows_stat_chunks(M, N), "bn_act_rows": h.tp3d_gemm_rows_stat_chunks(M, N)}[p.kernel]
        assert p.chunks == want > 0, ctx
        assert (p.kernel in ("x3_identity", "narrow", "rows")) == (l == 0), ctx
        assert (p.reverse is None) == (p.kernel in ("rows", "bn_act_rows")), ctx
        assert p.kernel != "narrow" or h.tp3d_gemm_tn_bn_narrow_serves(M, N, K), ctx
        formed = b.wgrad in ("x3_act", "x3_act_red")  # the loader waves form the activated rows: nothing was kept for them
        assert formed == (l > 0 and not p.keep_act), ctx
        assert not formed or (h.tp3d_gemm_tn_x3_serves(M, N, K) and b.terms), ctx
        assert (b.wgrad is not None) == bool(need_w[l]), ctx
        assert b.wgrad != "x3" or h.tp3d_gemm_tn_x3_serves(M, N, K), ctx
        assert b.wgrad_chunks == (h.tp3d_gemm_tn_x3_red_chunks(M, N, K) if b.wgrad == "x3_act_red" else 0), ctx
        assert b.wgrad != "x3_act_red" or (b.wgrad_chunks > 0 and b.terms == 6 and b.kind == "loader"), ctx
        from_above = b.kind != "passes" and b.reduce_rev is None
        assert from_above == (l + 1 < L and plan[l + 1].bwd.wgrad == "x3_act_red"), ctx
        ncol = b.cols[1] if b.cols else K
        assert b.cols is None or (l == 0 and b.cols == cols), ctx
        assert b.kind != "loader" or (h.tp3d_gemm_rows_bnbwd_sp_serves(M, ncol, N) and b.dx and b.dx_rev is not None), ctx
        assert b.kind != "narrow" or (l == 0 and not b.dx and b.wgrad == "narrow" and h.tp3d_gemm_tn_bn_narrow_serves(M, N, K)), ctx
        assert b.dx == (l > 0 or need_in) or b.kind == "narrow", ctx
        assert b.write_dY == {"loader": b.wgrad is not None, "narrow": False, "passes": True}[b.kind], ctx


def _sweep_chains(rows):
    for M, K0, widths, pool, need_in in itertools.product(rows, [c for c in CHANNELS if c % 4 == 0 and c <= 516], WIDTHS, (0, 64, 32),
                                                          (False, True)):
        if pool and M % pool:
            continue
        for cols in (None, (3, K0 - 4), (0, K0 - 4)) if K0 > 4 else (None,):
            yield M, K0, widths, pool, need_in, [True] * len(widths), cols
        yield M, K0, widths, pool, need_in, [l % 2 == 0 for l in range(len(widths))], None


def test_forward_and_backward_parts_of_every_plan_agree():
    """what the backward part relies on is what the forward part prepared, for every shape and every chain switch"""
    for case in _sweep_chains(ROWS[::2]):
        _check_couplings(*case, fused._plan_chain(*case[:4], True, *case[4:]))
    for name, value in CHAIN_SWITCHES:
        with _switch(name, value):
            for case in _sweep_chains([M for M in ROWS if M >= 65536][::3]):
                _check_couplings(*case, fused._plan_chain(*case[:4], True, *case[4:]))


def test_plan_without_gradient_request_keeps_nothing():
    for M, K0, widths, pool, need_in, need_w, cols in _sweep_chains(ROWS[::4]):
        plan = fused._plan_chain(M, K0, widths, pool, False, need_in, need_w, cols)
        assert all(p.bwd is None and not p.keep_act for p in plan), (M, K0, widths)
        # the forward kernels are those of the plan with a gradient request, where that one keeps no activated rows either
        full = fused._plan_chain(M, K0, widths, pool, True, need_in, need_w, cols)
        assert [p.kernel for p in plan] == [p.kernel for p in full] or any(p.keep_act for p in full), (M, K0, widths)


def _expected_route(M, Kp, Cout, training, pool_ns, want_grad):
    """the conditions of the five paths, each as one flat predicate"""
    h = _lib.load()
    skinny = M >= fused.SKINNY_MIN_ROWS and Kp <= fused.SKINNY_MAX and Cout <= fused.SKINNY_MAX
    served = (fused.USE_ROWS_GEMM and Cout >= fused.ROWS_GEMM_MIN_COLS and (fused.ROWS_GEMM_NARROW or not 0 < Cout % 128 <= 64)
              and Kp % 4 == 0 and not (((M + 127) // 128) * ((Cout + 127) // 128) < 128 and 512 <= Kp < 1024))
    stats = training and h.tp3d_gemm_rows_workspace_floats(M, Cout, Kp) == 0
    skinny_bnact = skinny and not training and not want_grad
    rows_epi = (not skinny_bnact and served and fused.ROWS_GEMM_EPILOGUE and fused.ROWS_GEMM_WITHOUT_STATS and not training
                and not pool_ns and not want_grad)
    rows = not skinny_bnact and not rows_epi and served and (stats or fused.ROWS_GEMM_WITHOUT_STATS)
    if skinny_bnact:
        return "skinny_bnact", False
    if rows_epi:
        return "rows_epi", False
    if rows:
        return "rows", stats
    return ("skinny" if skinny else "library"), False


LAYER_SWITCHES = [("USE_ROWS_GEMM", False), ("ROWS_GEMM_WITHOUT_STATS", False), ("ROWS_GEMM_EPILOGUE", False), ("ROWS_GEMM_NARROW", False)]


def _sweep_layers(rows):
    seen = set()
    for args in itertools.product(rows, CHANNELS, CHANNELS, (True, False), (0, 64), (True, False)):
        got = fused._layer_route(*args)
        assert got == _expected_route(*args), (args, got)
        seen.add(got)
    return seen


def test_layer_route_matches_the_conditions_of_each_path():
    seen = _sweep_layers(ROWS[::2])
    assert seen == {("skinny_bnact", False), ("rows_epi", False), ("rows", True), ("rows", False), ("skinny", False), ("library", False)}
    for name, value in LAYER_SWITCHES:
        with _switch(name, value):
            _sweep_layers(ROWS[::5])


def test_layer_route_of_known_layers():
    route = fused._layer_route
    assert route(524288, 128, 10, True, 0, True) == ("library", False)       # the class scores
    assert route(1048576, 8, 16, True, 0, True) == ("skinny", False)         # an edge MLP layer
    assert route(1048576, 8, 16, False, 0, False) == ("skinny_bnact", False)
    assert route(65536, 256, 64, False, 0, False) == ("rows_epi", False)
    assert route(65536, 256, 64, False, 0, True) == ("rows", False)
    h = _lib.load()
    for M, Kp, Cout in itertools.product(ROWS[::3], CHANNELS, CHANNELS):
        for training in (True, False):
            path, stats = route(M, Kp, Cout, training, 0, True)
            assert stats == (path == "rows" and training and h.tp3d_gemm_rows_workspace_floats(M, Cout, Kp) == 0), (M, Kp, Cout)
