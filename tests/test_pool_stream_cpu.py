"""The streaming slot pool's schedule restated on the host
(magpie_amd.dist.simulate_pool_stream): per round, which utterance gets a chunk of how many
frames and which ends, counted by hand, and the same loop's iteration count against
simulate_pool with poll = frames_per_chunk."""
import pytest


def test_rounds_counted_by_hand():
    from magpie_amd.dist import simulate_pool_stream
    # frames 4, 9, 2 through 2 slots at 4 frames per chunk, budget 48: an utterance that stops
    # at EOS holds its slot for frames + 1 iterations. Round 1 (iterations 1..4): both slots a
    # full chunk. Round 2 (5..8): utterance 0's EOS comes in iteration 5, nothing is left of
    # it, so it only ends, and utterance 2 is installed in slot 0; utterance 1 a full chunk.
    # Round 3 (9..12): slot 0 first, utterance 2's two frames and its end, then utterance 1's
    # ninth frame and its end.
    it, rounds = simulate_pool_stream([4, 9, 2], slots=2, fpc=4, max_dec_steps=48)
    assert rounds == [[(0, 4), (1, 4)], [(0, 0), (1, 4)], [(2, 2), (2, 0), (1, 1), (1, 0)]]
    assert it == 12


@pytest.mark.parametrize("fpc", [3, 4])
def test_pool_mix_chunks_and_iterations(fpc):
    from magpie_amd.dist import simulate_pool, simulate_pool_stream
    frames = [4, 4, 48, 48, 48, 5, 4, 39, 17, 48]
    it, rounds = simulate_pool_stream(frames, slots=4, fpc=fpc, max_dec_steps=48)
    assert it == simulate_pool(frames, 4, fpc, 48)[0] == fpc * len(rounds)
    chunks = {u: [] for u in range(len(frames))}
    ends = {u: 0 for u in range(len(frames))}
    for events in rounds:
        for u, n in events:
            if n == 0:
                ends[u] += 1
            else:
                assert ends[u] == 0, f"utterance {u}: a chunk after its end notice"
                chunks[u].append(n)
    for u, f in enumerate(frames):
        assert chunks[u] == [fpc] * (f // fpc) + ([f % fpc] if f % fpc else []), (u, chunks[u])
        assert sum(chunks[u]) == f
        assert ends[u] == 1


def test_arguments():
    from magpie_amd.dist import simulate_pool_stream
    with pytest.raises(ValueError):
        simulate_pool_stream([2], slots=1, fpc=0, max_dec_steps=8)
    with pytest.raises(ValueError):
        simulate_pool_stream([9], slots=1, fpc=4, max_dec_steps=8)
    # more slots than utterances: the surplus slots do not exist; a budget hit has no EOS iteration
    assert simulate_pool_stream([8, 2], slots=4, fpc=4, max_dec_steps=8) == (8, [[(0, 4), (1, 2), (1, 0)], [(0, 4), (0, 0)]])
