"""The forward-only WN kernels (fst_wn_layer_infer / fst_wn_stack_infer), checked without a GPU: the launchers they share with the saving
entry points name exactly the instances we think, each on its side of ``save``, tests/test_gpu_wn_infer.py declares a case for each of them, and the header, the ctypes binding and the route
names agree on the new symbols."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_wn_infer as I  # noqa: E402
from test_wn_routes_cpu import CSRC, _body, _instances, fwd_launcher  # noqa: E402

from feature_level_style_transfer_for_tsc_amd import _lib, ops  # noqa: E402

FUSED = open(os.path.join(CSRC, "wn_fused.hip")).read()
HEADER = open(os.path.join(ROOT, "include", "fst_hip.h")).read()


def _launched(body: str) -> set:
    """The kernels a launcher's body hands to hipLaunchKernelGGL."""
    return {re.sub(r"\s+", "", k) for k in re.findall(r"hipLaunchKernelGGL\(\s*([A-Za-z_0-9]+(?:<[^<>()]*>)?)\s*,", body)}


def test_the_launchers_name_exactly_the_infer_kernels():
    # each pair of entry points shares one launcher (fwd_launcher: the infer entry points pass save = false and do nothing else,
    # the saving ones save = true), and inside it the kernels are named on their own side of that selection only
    (layer_save, layer, layer_rest), (stack_save, stack, stack_rest) = fwd_launcher("layer"), fwd_launcher("stack")
    assert _launched(layer) == {"wn_layer_infer_kernel<4>", "wn_layer_infer_kernel<8>"} == _instances(layer, "wn_layer_infer_kernel")
    assert _launched(stack) == {"wn_stack_infer_kernel"}
    for side in (layer, stack):                                # neither can reach a saving kernel
        assert "wn_layer_fwd_kernel" not in side and "wn_stack_fwd_kernel" not in side
    # and the saving sides are as the saving launchers were: none of them launches an infer kernel
    assert _launched(layer_save) == {"wn_layer_fwd_kernel<4>", "wn_layer_fwd_kernel<8>"} == _instances(layer_save, "wn_layer_fwd_kernel")
    assert _launched(stack_save) == {"wn_stack_fwd_kernel"}
    for side in (layer_save, stack_save):
        assert "infer" not in side.lower()
    for rest in (layer_rest, stack_rest):                      # no kernel, no launch and no route family outside the selection
        assert "_kernel" not in rest and "hipLaunchKernelGGL" not in rest and "FST_WN_ROUTE" not in rest
    assert "FST_WN_ROUTE_LAYER_INFER" in layer and "FST_WN_ROUTE_LAYER_FWD" in layer_save
    assert "FST_WN_ROUTE_STACK_INFER" in stack and "FST_WN_ROUTE_STACK_FWD" in stack_save
    whole = _body(FUSED, "static int wn_layer_fwd_launch(") + _body(FUSED, "static int wn_stack_fwd_launch(")
    assert _launched(whole) == _launched(layer) | _launched(layer_save) | _launched(stack) | _launched(stack_save)
    # the infer kernels are the saving tile body with the stores compiled out, nothing else
    assert re.search(r"wn_fwd_tile<NW, false>\(", FUSED) and re.search(r"wn_fwd_tile<8, false>\(", FUSED)
    assert re.search(r"template <int NW, bool SAVE = true>\s*\n__device__ __forceinline__ void wn_fwd_tile\(", FUSED)


def test_every_infer_kernel_has_a_declared_case():
    declared = {f"wn_layer_infer_kernel<{c.nw}>" for c in I.LI_CASES}
    assert declared == {"wn_layer_infer_kernel<4>", "wn_layer_infer_kernel<8>"}
    for c in I.LI_CASES:                                       # each case is declared for the instance its shape gives (256 CUs)
        route = I.layer_infer_expect(I._batch(c.B, 256), c.L)
        assert route[1] == c.nw and ops.wn_route_kernel_name(route) == f"wn_layer_infer_kernel<{c.nw}>", c.id
    assert I.SI_CASES and all(ops.wn_route_kernel_name(I.stack_infer_expect(I._batch(c.B, 256), c.L, c.nl)) == "wn_stack_infer_kernel"
                              for c in I.SI_CASES)


def test_the_case_lists_span_what_the_issue_asks_for():
    four = [c for c in I.LI_CASES if c.nw == 4]
    forms = {(a, b) for a in (True, False) for b in (True, False)}
    assert {(c.B, c.L) for c in four} == {(2, 160)} and 160 % 128 != 0
    for nh in ((8, 3), (127, 32), (120, 25)):
        for dil_ok in (lambda d: d == 1, lambda d: d >= 160):
            assert {(c.first, c.last) for c in four if (c.n, c.h) == nh and dil_ok(c.dil)} == forms, nh
    eight = [c for c in I.LI_CASES if c.nw == 8]
    assert {(c.B, c.L, c.n) for c in eight} == {("cus", 256, 8)} and {(c.first, c.last) for c in eight} == forms
    assert {1, 2, 3, 8} <= {c.nl for c in I.SI_CASES if (c.B, c.n, c.L) == ("cus+1", 8, 256)}
    assert any((c.n, c.h, c.B, c.L, c.nl) == (120, 25, 256, 512, 8) for c in I.SI_CASES)
    assert any(c.L > 256 for c in I.SI_CASES)                  # more than one tile per sequence and layer


def test_header_binding_and_route_names_agree():
    decl = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("fst_wn_layer_infer", "fst_wn_stack_infer"):
        assert name in _lib.EXPORTED_SYMBOLS and re.search(r"\bint " + name + r"\(", decl), name
        assert f'extern "C" int {name}(' in FUSED
    # the argument lists: the saving entry points' without ts (and acts)
    sig = _lib._SIGNATURES
    fwd, inf = sig["fst_wn_layer_fwd"][1], sig["fst_wn_layer_infer"][1]
    assert inf == fwd[:6] + fwd[8:] and sig["fst_wn_layer_infer"][0] is sig["fst_wn_layer_fwd"][0]
    fwd, inf = sig["fst_wn_stack_fwd"][1], sig["fst_wn_stack_infer"][1]
    assert inf == fwd[:4] + fwd[5:]
    params = lambda name: [p.strip().split()[-1].lstrip("*") for p in
                           re.search(r"\bint " + name + r"\((.*?)\);", decl, flags=re.S).group(1).split(",")]
    assert params("fst_wn_layer_infer") == [p for p in params("fst_wn_layer_fwd") if p not in ("ts", "acts")]
    assert params("fst_wn_stack_infer") == [p for p in params("fst_wn_stack_fwd") if p != "ts"]
    assert len(params("fst_wn_layer_infer")) == len(sig["fst_wn_layer_infer"][1])
    assert len(params("fst_wn_stack_infer")) == len(sig["fst_wn_stack_infer"][1])
    # route families
    fam = dict(re.findall(r"#define FST_WN_ROUTE_(\w+)\s+(\d+)", HEADER))
    assert int(fam["LAYER_INFER"]) == ops.WN_ROUTE_LAYER_INFER and int(fam["STACK_INFER"]) == ops.WN_ROUTE_STACK_INFER
    assert len(set(fam.values())) == len(fam)                  # (LEN included: no family shares a number)
    assert ops.wn_route_kernel_name((ops.WN_ROUTE_LAYER_INFER, 4) + (0,) * 10) == "wn_layer_infer_kernel<4>"
    assert ops.wn_route_kernel_name((ops.WN_ROUTE_STACK_INFER, 8) + (0,) * 10) == "wn_stack_infer_kernel"
    assert "FST_WN_ROUTE_LAYER_INFER" in FUSED and "FST_WN_ROUTE_STACK_INFER" in FUSED
    ver = int(re.search(r"#define FST_ABI_VERSION (\d+)", HEADER).group(1))
    assert ver == _lib.ABI_VERSION >= 20


def test_the_forward_saves_only_when_something_requires_a_gradient():
    """The autograd nodes pass ``save=any(ctx.needs_input_grad)`` (grad mode is off inside a Function's forward, so it cannot be
    asked there) and FST_WN_INFER=0 keeps the saving launches."""
    import inspect
    for fn in (ops.WNFn, ops.FlowFn):
        assert "save=any(ctx.needs_input_grad)" in inspect.getsource(fn.forward), fn.__name__
    assert "save" in inspect.signature(ops._wn_forward).parameters and inspect.signature(ops._wn_forward).parameters["save"].default is True
    old = os.environ.pop("FST_WN_INFER", None)
    try:
        assert ops.wn_infer_enabled()
        os.environ["FST_WN_INFER"] = "0"
        assert not ops.wn_infer_enabled()
    finally:
        os.environ.pop("FST_WN_INFER", None)
        if old is not None:
            os.environ["FST_WN_INFER"] = old
