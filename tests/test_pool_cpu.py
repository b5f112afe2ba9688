"""Continuous batching, the host side without a GPU: the schedule restated in Python
(magpie_amd.dist.simulate_pool) against hand-counted cases, the claim logic of
synthesize_pool over a fake device, and the new C-ABI symbols."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- simulate_pool: (iterations, useful slot-iterations), counted by hand
def test_simulate_one_slot():
    from magpie_amd.dist import simulate_pool
    # frames 3, 10, 2 at poll 4, budget 20: an utterance of f frames holds the slot f + 1
    # iterations (the EOS iteration emits nothing). 3 -> done after iteration 4, seen at 4;
    # 10 runs 5..15, seen at 16; 2 runs 17..19, seen at 20.
    assert simulate_pool([3, 10, 2], slots=1, poll=4, max_dec_steps=20) == (20, 15)
    # the streaming form emits the EOS frame: f frames are f iterations. 3 -> seen at 4;
    # 10 runs 5..14, seen at 16; 2 runs 17..18, seen at 20.
    assert simulate_pool([3, 10, 2], slots=1, poll=4, max_dec_steps=20, emit_eos=True) == (20, 15)
    # 4 frames + the EOS iteration = 5 > 4: seen at 8, not at 4
    assert simulate_pool([4], slots=1, poll=4, max_dec_steps=20) == (8, 4)
    assert simulate_pool([4], slots=1, poll=4, max_dec_steps=20, emit_eos=True) == (4, 4)


def test_simulate_budget_hit():
    from magpie_amd.dist import simulate_pool
    # an utterance that runs into max_dec_steps = 8 stops with its 8th frame: 8 iterations,
    # no EOS iteration. Seen at 8; the next (2 frames, 3 iterations: 9..11) is seen at 12.
    assert simulate_pool([8, 2], slots=1, poll=4, max_dec_steps=8) == (12, 10)
    # 7 frames under the same budget end on an EOS in iteration 8 as well
    assert simulate_pool([7, 2], slots=1, poll=4, max_dec_steps=8) == (12, 9)


def test_simulate_two_slots_same_poll():
    from magpie_amd.dist import simulate_pool
    # slots 0 and 1 hold 2 and 3 frames (3 and 4 iterations): both seen at poll 4 and
    # refilled in slot order, slot 0 with the 9-frame utterance (5..14, seen at 16), slot 1
    # with the 1-frame one (5..6, seen at 8, nothing left to install). Ends at 16.
    assert simulate_pool([2, 3, 9, 1], slots=2, poll=4, max_dec_steps=50) == (16, 15)
    # more slots than utterances: the surplus slots do not exist
    assert simulate_pool([2, 3], slots=8, poll=4, max_dec_steps=50) == (4, 5)


def test_simulate_poll_one():
    from magpie_amd.dist import simulate_pool
    # poll 1: a slot is refilled right after its last iteration. Slot 0: 2 frames (1..3),
    # then 4 frames (4..8); slot 1: 5 frames (1..6), then 1 frame (7..8). Ends at 8.
    assert simulate_pool([2, 5, 4, 1], slots=2, poll=1, max_dec_steps=50) == (8, 12)
    with pytest.raises(ValueError):
        simulate_pool([2], slots=0, poll=1, max_dec_steps=50)
    with pytest.raises(ValueError):
        simulate_pool([51], slots=1, poll=1, max_dec_steps=50)


# ---- synthesize_pool over a fake device
class FakeDevice:
    """synthesize_queue's contract without a GPU: runs whatever next() hands out until it
    returns -1, noting the order; an utterance's codes are its index and text length."""

    def __init__(self):
        self.claims = []

    def synthesize_queue(self, tokens, speakers=None, slots=8, poll=8, next=None, **kw):
        import numpy as np
        from magpie_amd import QueueResult
        codes = [None] * len(tokens)
        nf = np.full(len(tokens), -1, np.int32)
        while True:
            u = next()
            if u < 0:
                break
            assert codes[u] is None, "claimed twice"
            self.claims.append(u)
            codes[u] = np.full((1, 8), 1000 * u + len(tokens[u]), np.int32)
            nf[u] = 1
        return QueueResult(codes, nf, iterations=len(self.claims), slots=slots, refills=max(0, len(self.claims) - slots),
                           useful_slot_iters=len(self.claims), decode_ms=0.0)


TEXTS = [[0] * n for n in (5, 9, 2, 9, 7, 1, 12)]


def test_pool_claims_every_index_once_longest_first():
    from magpie_amd.dist import gather_results, longest_first, synthesize_pool
    dev = FakeDevice()
    mine = synthesize_pool(dev, TEXTS, slots=2, poll=4)
    assert dev.claims == longest_first(TEXTS) == [6, 1, 3, 4, 0, 2, 5]
    assert sorted(mine) == list(range(len(TEXTS)))
    got = gather_results(mine, len(TEXTS))  # shaped like synthesize_queue's result
    assert [int(c[0, 0]) for c in got] == [1000 * i + len(t) for i, t in enumerate(TEXTS)]
    assert mine.stats.refills == len(TEXTS) - 2 and mine.stats.codes == []
    with pytest.raises(ValueError):
        synthesize_pool(dev, TEXTS, speakers=[0], slots=2)


def test_pool_two_ranks_share_one_queue():
    """Two fake ranks of one process on one WorkQueue, their claims interleaved: every
    position goes to exactly one of them, in longest-first order overall."""
    from magpie_amd.dist import WorkQueue, longest_first, synthesize_pool
    q = WorkQueue(len(TEXTS))
    order = longest_first(TEXTS)

    class Rank(FakeDevice):
        """takes `quota` claims, then lets the other rank run before it goes on"""
        def __init__(self, quota, other=None):
            super().__init__()
            self.quota, self.other, self.result = quota, other, None

        def synthesize_queue(self, tokens, speakers=None, slots=8, poll=8, next=None, **kw):
            rank = self

            def metered():
                if len(rank.claims) == rank.quota and rank.other is not None and rank.other.result is None:
                    rank.other.result = synthesize_pool(rank.other, TEXTS, slots=2, queue=q)
                return next()
            return super().synthesize_queue(tokens, speakers, slots, poll, metered, **kw)

    b = Rank(quota=3)
    a = Rank(quota=2, other=b)
    mine_a = synthesize_pool(a, TEXTS, slots=2, queue=q)
    mine_b = b.result
    assert a.claims == order[:2] and b.claims == order[2:]  # b drained the queue while a waited
    assert not set(mine_a) & set(mine_b)
    assert sorted(list(mine_a) + list(mine_b)) == list(range(len(TEXTS)))


# ---- ABI
def test_queue_symbols_and_stats_layout():
    import magpie_amd as ma
    lib = ma.load_library()
    assert hasattr(lib, "mp_hip_decode_queue")
    names = {s for s, _, _ in ma.SYMBOLS}
    assert "mp_hip_decode_queue" in names
    hdr = open(os.path.join(REPO, "include", "magpie_hip.h")).read()
    assert re.search(r"typedef int \(\*mp_next_cb\)\(void \*user\);", hdr)
    assert re.search(r"typedef void \(\*mp_done_cb\)\(int utt, const int32_t \*codes[^,]*, int n_frames, void \*user\);", hdr)
    # struct { int iterations, slots, refills; long long useful_slot_iters; double decode_ms; }:
    # 3 ints, 4 bytes of padding to the 8-byte member, 8 + 8
    s = ma.mp_queue_stats
    assert [f[0] for f in s._fields_] == ["iterations", "slots", "refills", "useful_slot_iters", "decode_ms"]
    assert ctypes.sizeof(s) == 32
    assert s.useful_slot_iters.offset == 16 and s.decode_ms.offset == 24
    # without a model (or a device) the call refuses instead of running
    assert lib.mp_hip_decode_queue(None, None, None, None, 1, 1, 1, 8, None, ctypes.cast(None, ma.NEXT_CB),
                                   ctypes.cast(None, ma.DONE_CB), None, None) == -1
    # the C++ drop-in layer exports its queue call from the same library
    import subprocess
    out = subprocess.run(["nm", "-DC", ma.LIB_PATH], capture_output=True, text=True).stdout
    assert "magpie_synthesize_codes_queue(magpie_context*, int const* const*, int const*, int, int, " in out
