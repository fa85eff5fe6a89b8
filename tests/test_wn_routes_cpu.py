"""Completeness of tests/test_gpu_wn_routes.py, without a GPU: every kernel instance the pickers of csrc/wn_wgrad.hip and
csrc/wn_fused.hip can launch has a case there that is declared for it, and every case's declaration is what the launcher's
geometry (restated in that module, asserted against the library's route record on the GPU) gives for its shape."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_wn_routes as R  # noqa: E402

CSRC = os.path.join(ROOT, "feature_level_style_transfer_for_tsc_amd", "csrc")


def _body(text: str, head: str) -> str:
    """The body of the function whose definition starts with ``head`` (up to the first line that is a lone closing brace)."""
    start = text.index(head)
    return text[start: text.index("\n}\n", start)]


def _instances(body: str, kernel: str) -> set:
    return {f"{kernel}<{', '.join(a.strip() for a in args.split(','))}>" for args in re.findall(kernel + r"<([^<>()]*)>", body)}


def _until(text: str, i: int, stops: str, pair: str) -> int:
    """From ``i`` on, the index of the first character of ``stops`` outside any ``pair`` of brackets — or of the bracket that
    closes the pair ``i`` is in."""
    depth = 0
    while depth > 0 or (text[i] not in stops and text[i] != pair[1]):
        depth += (text[i] == pair[0]) - (text[i] == pair[1])
        i += 1
    return i


def _save_sides(body: str):
    """A launcher that takes ``bool save``, split by that selection: (the text reachable only when saving, only when not, the
    rest).  The selections are the arms of every ``save ? x : y`` (a nested ?: stands in parentheses) and the blocks of every
    ``if (save) { } else { }``."""
    yes, no, rest, pos = "", "", "", 0
    for m in re.finditer(r"\bsave \?|\bif \(save\) \{", body):
        assert m.start() >= pos, "a save selection inside a save selection"
        if m.group().endswith("?"):
            mid = _until(body, m.end(), ":", "()")
            assert body[mid] == ":"
            end = _until(body, mid + 1, ",;", "()")
            arms, after = (body[m.end(): mid], body[mid + 1: end]), end
        else:
            mid = _until(body, m.end(), "", "{}")
            assert body[mid:].startswith("} else {")
            end = _until(body, mid + len("} else {"), "", "{}")
            arms, after = (body[m.end(): mid], body[mid + len("} else {"): end]), end + 1
        rest, yes, no, pos = rest + body[pos: m.start()], yes + arms[0], no + arms[1], after
    return yes, no, rest + body[pos:]


def fwd_launcher(form: str):
    """(saving side, no-save side, rest) of the launcher behind fst_wn_<form>_fwd and fst_wn_<form>_infer (form: layer / stack),
    after checking that these two pass save = true and save = false and do nothing else."""
    fused = open(os.path.join(CSRC, "wn_fused.hip")).read()
    for name, save in ((f"fst_wn_{form}_fwd", "true"), (f"fst_wn_{form}_infer", "false")):
        stmts = [s.strip() for s in _body(fused, f'extern "C" int {name}(').split("{", 1)[1].split(";") if s.strip()]
        assert len(stmts) == 2 and stmts[0] == "fst_wn_clear_route()", (name, stmts)
        assert re.match(r"return wn_" + form + r"_fwd_launch\(\"" + name + r"\", " + save + r",[^()]*\)$", stmts[1]), (name, stmts[1])
    return _save_sides(_body(fused, f"static int wn_{form}_fwd_launch("))


def source_instances():
    wgrad = open(os.path.join(CSRC, "wn_wgrad.hip")).read()
    ww = _instances(_body(wgrad, "static int ww_launch("), "wn_wgrad_kernel")
    tz = _instances(_body(wgrad, 'extern "C" int fst_dense_tap_wgrad('), "tz_wgrad_kernel")
    fw = _instances(fwd_launcher("layer")[0], "wn_layer_fwd_kernel")      # what fst_wn_layer_fwd can reach: the saving side
    return ww, tz, fw


def test_the_pickers_have_the_instances_we_think():
    ww, tz, fw = source_instances()
    assert len(ww) == 8 and len(tz) == 4 and fw == {"wn_layer_fwd_kernel<4>", "wn_layer_fwd_kernel<8>"}, (sorted(ww), sorted(tz), sorted(fw))


def _wgrad_declared():
    return ({c.inst for c in R.WIN_CASES} | {c.inst for c in R.WRS_CASES} | {c.inst for c in R.TAP_CASES} | {c.inst for c in R.NT_CASES})


def test_every_instance_has_a_case():
    ww, tz, fw = source_instances()
    got = _wgrad_declared()
    assert got == ww, f"not covered: {sorted(ww - got)}; not an instance: {sorted(got - ww)}"
    got = {c.inst for c in R.TZ_CASES}
    assert got == tz, f"not covered: {sorted(tz - got)}; not an instance: {sorted(got - tz)}"
    got = {f"wn_layer_fwd_kernel<{c.nw}>" for c in R.FW_CASES}
    assert got == fw, f"not covered: {sorted(fw - got)}"


def test_every_case_is_declared_for_the_instance_its_shape_gives():
    name = R.ops.wn_route_kernel_name
    for c in R.WIN_CASES:
        assert name(R.wn_wgrad_expect(0, c.B, c.L, c.n, c.h, False, c.n_sets, c.dil)[0]) == c.inst, c.id
    for c in R.WRS_CASES:
        assert name(R.wn_wgrad_expect(1, c.B, c.L, c.n, 0, c.last, c.n_sets, 4)[0]) == c.inst, c.id
    for c in R.TAP_CASES:
        assert name(R.tap_wgrad_expect(c.B, c.L, c.M, c.C, c.ntaps, c.dil, c.pad)[0]) == c.inst, c.id
    for c in R.NT_CASES:
        route = R.nt_gemm_expect(c.M, c.N, c.K, c.epi > 0)[0]
        assert name(route) == c.inst and route[10] == int(not c.direct), c.id
    for c in R.TZ_CASES:
        assert name(R.tz_expect(c.B, c.L, c.M, c.C, c.K)[0]) == c.inst, c.id
    for c in R.FW_CASES:
        assert R.layer_fwd_expect(c.B, c.L)[1] == c.nw, c.id


def test_the_case_lists_span_what_the_issue_asks_for():
    win = R.WIN_CASES
    routes = [R.wn_wgrad_expect(0, c.B, c.L, c.n, c.h, False, c.n_sets, c.dil)[0] for c in win]
    assert {r[6] for r in routes} == {1, 2, 3}                                     # k-row groups
    assert {c.n_sets for c in win} == {1, 2, 3} and {c.n_sets for c in R.WRS_CASES} == {1, 2, 3}
    assert any(c.n_sets > 1 and (c.B * c.L // 32) % (r[5] // c.n_sets) for c, r in zip(win, routes))    # uneven tile shares
    assert any(c.B == 1 and c.L == 32 and r[5] == c.n_sets for c, r in zip(win, routes))              # K split clamped by the tiles
    assert {1, 2, 3, 4, 8} <= {c.dil for c in win} and any(c.dil >= c.L for c in win)
    for inst in (R.F1, R.P1):                                                        # the leftover k-row with several sets
        assert any(c.inst == inst and c.n_sets > 1 for c in win), inst
    assert {1, 32} <= {c.h for c in win} and {1, 127} <= {c.n for c in win}
    assert {c.last for c in R.WRS_CASES} == {True, False}
    assert any(c.inst == R.F0 for c in R.TAP_CASES) and any(R.cdiv(c.ntaps * c.C, 32) == 18 for c in R.TAP_CASES)
    assert {c.M for c in R.TZ_CASES} >= {32, 33, 64, 65, 96, 97, 128, 129, 224, 225} and {c.K for c in R.TZ_CASES} >= {64, 65}
    assert any(c.direct for c in R.NT_CASES) and any(c.M == 255 for c in R.NT_CASES) and {c.epi for c in R.NT_CASES} == {0, 1, 2}
    assert {(c.first, c.last) for c in R.FW_CASES} == {(a, b) for a in (True, False) for b in (True, False)}
    assert {c.acts for c in R.FW_CASES if c.nw == 4} == {True, False} == {c.acts for c in R.FW_CASES if c.nw == 8}
    assert any(c.nw == 4 and c.L % 128 for c in R.FW_CASES)
    assert {1, 16, 64, 128, "max"} <= {c.dil for c in R.DG_CASES} and {c.res for c in R.DG_CASES} == {True, False}
    assert any(c.B * R.cdiv(c.L, 512) > 256 for c in R.DG_CASES) and any(c.B * R.cdiv(c.L, 512) <= 256 for c in R.DG_CASES)


def test_no_dilation_gets_a_three_slot_dgrad_ring():
    """fst_wn_layer_dgrad takes 2 ring slots without asking whether 3 would fit 160 KiB: with 512-sample tiles a slot is
    61 696 bytes at dilation 1 and grows with the dilation, so they never do."""
    fused = open(os.path.join(CSRC, "wn_fused.hip")).read()
    assert re.search(r"#define DG_TN \(8 \* 32 \* DG_NCB\)", fused) and re.search(r"#define DG_NCB 2\b", fused)
    assert re.search(r"\*nblkw = \(DG_TN \+ 2 \* dil \+ 3 \+ 31\) / 32;", fused) and "*slot = DG_A_BYTES + 2 * *gsw;" in fused
    assert R.dgrad_slot(1) == 61696 and R.dgrad_ring_slots(1) == 2
    assert all(R.dgrad_slot(d + 1) >= R.dgrad_slot(d) for d in range(1, 200))


# the (n, h) of every fst_wn_wgrad_in shape and the (M, C, ntaps) of every fst_tap_wgrad shape in the suite before
# test_gpu_wn_routes.py (test_gpu_full_size.py::test_time_as_k_weight_gradient*, test_gpu_kernels.py::test_few_tap_dense_*)
_EARLIER_IN = [(120, 25), (33, 31), (8, 3), (16, 5), (127, 32), (16, 16), (48, 5)]
_EARLIER_TAP = [(50, 225, 2), (33, 70, 3), (8, 64, 4), (256, 130, 3)]


def test_the_earlier_case_lists_missed_two_instances():
    name = R.ops.wn_route_kernel_name
    got = {name(R.wn_wgrad_expect(0, 2, 64, n, h, False, 1, 4)[0]) for n, h in _EARLIER_IN}
    got |= {name(R.tap_wgrad_expect(2, 64, M, C, k, 4, 0)[0]) for M, C, k in _EARLIER_TAP}
    kt3 = {i for i in source_instances()[0] if i.startswith("wn_wgrad_kernel<2, 3,")}
    assert kt3 - got == {R.F0, R.P1}, sorted(kt3 - got)
