"""The decode iteration's launch list (build_iteration / build_lt, launched by launch_ops).

The list is built once per batch configuration; the graph capture, eager mode
(MAGPIE_EAGER=1) and the profiling API all launch that one list. Checked here:
  - it is the list the runtime launched before it had a builder: the names in order and
    the algorithmic bytes of tests/golden/op_lists.json (tools_dev/dump_op_lists.py run with
    that earlier library), for every weight mode, batch-size class and list-shaping knob;
  - eager mode launches what the graph replays: same list, same codes, same hidden bits;
  - the profiler replays the decode's own list and leaves the batch decodable.
2-layer models, 24-token prompts, 8 greedy frames.
"""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dump_op_lists", os.path.join(REPO, "tools_dev", "dump_op_lists.py"))
dol = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dol)

with open(os.path.join(REPO, "tests", "golden", "op_lists.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    if magpie_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return magpie_amd


@pytest.fixture(scope="module")
def graph_run(ma, small_model, f16_model, q8_model, q4_model):
    """case -> (result, names, bytes) of its graph-mode decode, run once per case."""
    paths = {"small": small_model, "f16": f16_model, "q8": q8_model, "q4": q4_model}
    done = {}

    def run(case, eager=False):
        if eager:
            return dol.run_case(ma, paths[dol.CASES[case][0]], case, eager=True)
        if case not in done:
            done[case] = dol.run_case(ma, paths[dol.CASES[case][0]], case)
        return done[case]
    return run


def test_golden_covers_every_case():
    assert sorted(GOLDEN) == sorted(dol.CASES)


@pytest.mark.parametrize("case", sorted(dol.CASES))
def test_op_list_is_the_recorded_one(graph_run, case):
    _, names, nbytes = graph_run(case)
    want = GOLDEN[case]
    assert names == want["names"]
    # sums of integer products with 34/32 and 18/32: only a reassociated sum could move them, by ulps
    for i, (got, ref) in enumerate(zip(nbytes, want["bytes"])):
        assert abs(got - ref) <= 1e-9 * abs(ref), (i, names[i], got, ref)


@pytest.mark.parametrize("case", ["f32_b1", "bf16_b8", "q8_b4"])
def test_eager_launches_what_the_graph_replays(graph_run, case):
    rg, names_g, _ = graph_run(case)
    re_, names_e, _ = graph_run(case, eager=True)
    assert names_e == names_g
    print(f"{case}: eager vs graph hidden max diff per frame",
          np.abs(re_.hidden - rg.hidden).max(axis=(0, 2)))
    for b in range(len(rg.codes)):
        assert np.array_equal(re_.codes[b], rg.codes[b]), f"slot {b} codes"
    assert np.array_equal(re_.hidden, rg.hidden)


@pytest.mark.parametrize("case", ["f32_b1", "q8_b1"])
def test_profiler_replays_the_decode_list(ma, graph_run, small_model, q8_model, case):
    path = {"small": small_model, "q8": q8_model}[dol.CASES[case][0]]
    dev = ma.Device(path, weights=dol.CASES[case][1])
    toks = [ma.synthetic_tokens(24, seed=9100)]
    kw = dict(speakers=[0], max_dec_steps=8, ignore_eos=True, trace=True)
    r1 = dev.synthesize(toks, **kw)
    names = dev.ops()
    us = dev.profile_ops(iters=2)
    r2 = dev.synthesize(toks, **kw)
    dev.close()
    assert names == graph_run(case)[1]
    assert len(us) == len(names) and np.all(np.isfinite(us)) and np.all(us > 0), us
    # the hidden trace: the rows of the decoded frames (the profiler's replays run on as
    # further steps, and a step below max_dec_steps + 1 writes its trace row)
    n = int(r1.n_frames[0])
    print(f"{case}: hidden max diff per frame", np.abs(r2.hidden - r1.hidden).max(axis=(0, 2)))
    assert n == 8 and np.array_equal(r2.codes[0], r1.codes[0])
    assert np.array_equal(r2.hidden[:, :n], r1.hidden[:, :n])
