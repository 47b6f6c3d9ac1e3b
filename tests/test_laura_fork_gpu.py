"""DecodeSlots.fork / rewind on the GPU: a slot takes up another slot's utterance (or its own) as it stood after its first `keep`
generated tokens -- a device copy of cache positions, token and log-probability rows, the counters set, the LM's input layer run on
token keep - 1 -- and goes on with its own sampling, seed and max_length.  No tolerance anywhere:

(a) with the source's own sampling and seed the destination's complete result is the source's (test_laura_slots_gpu.same: length,
    tokens and every log-probability row by torch.equal);
(b) after any fork or rewind the per-step log-probabilities are those of a slot that ``start``s the same prompt alone in a session of
    the same S = 4, in the same slot, with forced= the fork's final tokens.

Prompt 0 of laura_tiny_b3 has 7 text tokens: prefix lengths P = 9, 12, 13 (cont_len 0 / 3 / 4); the copy takes P + keep - 1
positions, which these and the keeps below make both a multiple of 4 and not."""
import pytest
import torch

from test_laura import MAN
from test_laura_slots_gpu import B3, EOS, prompts, run_to_end, same, texts_of
from test_laura_start_from_gpu import CAP, S, STEPS, alone, prompt0

pytestmark = pytest.mark.gpu


def step_until_done(s, slots, limit=64):
    """step(1) until none of `slots` is running; nothing is taken"""
    for _ in range(limit):
        st = s.step(1)
        if all(st.get(i) != "running" for i in slots):
            break
    assert all(st.get(i) == "done" for i in slots), st


def forced_alone(eng, slot, text, cont, got, cont_len):
    """property (b)'s right-hand side: ``start`` alone in `slot` with forced= the generated tokens of `got`, max_length = their number"""
    n = got[1] - cont_len
    assert n >= 1
    return n, alone(eng, None, slot, text, n, False, 0, cont, forced=got[0][cont_len:].cpu(), memo=False)


def assert_b(eng, slot, text, cont, got, cont_len):
    n, ref = forced_alone(eng, slot, text, cont, got, cont_len)
    assert ref[1] == got[1] and torch.equal(ref[0], got[0])
    assert ref[2].shape[0] == n and torch.equal(got[2][:n], ref[2]), float((got[2][:n] - ref[2]).abs().max())


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cont_len", [0, 3, 4])
def test_the_same_seed_replays_the_source(cont_len):
    eng, A, c, spec = prompt0(cont_len)
    P = A.shape[0] + 2 + cont_len
    assert P == {0: 9, 3: 12, 4: 13}[cont_len]
    ref = alone(eng, ("A", cont_len), 1, A, STEPS, True, 11, c)
    assert ref[1] - cont_len >= 7, "the source must still run after 6 steps"
    s = eng.open_decode(S, max_positions=CAP)
    s.start(1, A, A.shape[0], STEPS, sampling=True, seed=11, continual=c)
    st = s.step(6)                                                           # the start drew token 1, six steps six more
    assert st[1] == "running" and s.n_gen(1) == 7
    s.fork(0, 1, 6, sampling=True, seed=11)                                  # one below the source, two above
    s.fork(2, 1, None, sampling=True, seed=11)                               # everything: 7 tokens
    s.fork(3, 1, 3, STEPS, sampling=True, seed=11)
    assert [s.n_gen(i) for i in range(4)] == [6, 7, 7, 3]
    step_until_done(s, [0, 1, 2, 3])
    got = {i: s.take(i, return_logp=True) for i in (0, 2, 3)}
    s.fork(3, 1, 1, sampling=True, seed=11)                                  # the source has ended and is not taken
    s.fork(0, 1, 4, sampling=True, seed=11)
    got2 = run_to_end(s, [0, 1, 3])
    s.free()
    assert {(P + k - 1) % 4 for k in (7, 6, 4, 3, 1)} >= {0, 1}
    for slot, keep in ((0, 6), (2, 7), (3, 3)):
        assert same(got[slot], ref), (slot, keep)
    assert same(got2[3], ref), "keep = 1, from an ended source"
    assert same(got2[0], ref), "keep = 4, from an ended source"
    assert same(got2[1], ref), "the source, with five slots forked from it, is the source alone"


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_another_seed_and_mode_from_keep_on():
    eng, A, c, spec = prompt0(3)
    ref = alone(eng, ("A", 3), 1, A, STEPS, True, 11, c)
    s = eng.open_decode(S, max_positions=CAP)
    s.start(1, A, A.shape[0], STEPS, sampling=True, seed=11, continual=c)
    assert s.step(6)[1] == "running"
    modes = {0: (False, 0), 2: (5, 3), 3: (0.7, 9)}
    for slot, (sampling, seed) in modes.items():
        s.fork(slot, 1, 4, sampling=sampling, seed=seed)
    got = run_to_end(s, [0, 1, 2, 3])
    s.free()
    assert same(got[1], ref)
    differs = []
    for slot in modes:
        g = got[slot]
        assert g[1] >= 3 + 4 and torch.equal(g[0][: 3 + 4], ref[0][: 3 + 4]), slot      # prompt tokens and kept tokens [0, 4)
        assert torch.equal(g[2][:4], ref[2][:4]), slot
        assert_b(eng, slot, A, c, g, 3)
        differs.append(g[1] != ref[1] or not torch.equal(g[0], ref[0]))
    assert differs[1] or differs[2], "a seeded destination must leave the source's path after token 4"


# 3 ---------------------------------------------------------------------------------------------------------------------------
def rewound(eng, A, c, keep, sampling, seed):
    s = eng.open_decode(S, max_positions=CAP)
    s.start(2, A, A.shape[0], STEPS, sampling=True, seed=11, continual=c)
    step_until_done(s, [2])
    first_len = s.n_gen(2)
    s.rewind(2, keep, sampling=sampling, seed=seed)
    assert s.n_gen(2) == keep
    assert s.step(1)[2] in ("running", "done")                              # an ended slot runs again
    got = run_to_end(s, [2])[2]
    s.free()
    return got, first_len


def test_rewind_in_place():
    eng, A, c, spec = prompt0(4)
    ref = alone(eng, ("A", 4), 2, A, STEPS, True, 11, c)
    got, first_len = rewound(eng, A, c, 5, True, 11)
    assert first_len == ref[1] - 4 and same(got, ref), "(i) the same seed: the first result again"
    other, _ = rewound(eng, A, c, 5, True, 12)
    assert torch.equal(other[0][: 4 + 5], ref[0][: 4 + 5]) and torch.equal(other[2][:5], ref[2][:5])
    assert_b(eng, 2, A, c, other, 4)                                         # (ii)
    assert not torch.equal(other[2], ref[2]), "another seed draws other tokens within 7 steps"


def test_rewind_in_both_step_forms():
    eng, A, c, spec = prompt0(4)

    def both():
        got, _ = rewound(eng, A, c, 5, True, 11)
        mid, _ = rewound(eng, A, c, 1, 5, 7)
        return got, alone(eng, None, 2, A, STEPS, True, 11, c, memo=False), mid

    assert eng.set_persistent_step(True)
    try:
        assert not eng.set_persistent_step(False)
        got, ref, mid = both()
        assert same(got, ref), "kernel chain"
        assert_b(eng, 2, A, c, mid, 4)
    finally:
        assert eng.set_persistent_step(True)
    got, ref, mid = both()
    assert same(got, ref), "persistent step"
    assert_b(eng, 2, A, c, mid, 4)


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_a_source_that_ended_by_length():
    eng, A, c, spec = prompt0(4)
    short, long = alone(eng, ("A", 4), 1, A, 8, True, 11, c), alone(eng, ("A", 4), 1, A, STEPS, True, 11, c)
    assert short[1] == 4 + 8, "ends by length"
    s = eng.open_decode(S, max_positions=CAP)
    s.start(1, A, A.shape[0], 8, sampling=True, seed=11, continual=c)
    step_until_done(s, [1])
    assert s.n_gen(1) == 8
    s.fork(0, 1, None, STEPS, sampling=True, seed=11)                        # everything it has, and room to go on
    s.fork(3, 1, 5, sampling=True, seed=11)                                  # the source's max_length
    s.rewind(1, 4, sampling=True, seed=11)
    got = run_to_end(s, [0, 1, 3])
    s.free()
    assert got[0][2].shape[0] == STEPS and same(got[0], long), "what start gives with the larger max_length"
    assert same(got[3], short) and same(got[1], short)


def test_a_source_that_ended_on_eos():
    eng, Q, spec = prompts(EOS)
    assert MAN["cases"][EOS]["tokens"] == [6, 8]
    s = eng.open_decode(S, max_positions=CAP)
    for b in (0, 1):
        s.start(b, Q[b], Q[b].shape[0], 16, sampling=False)
    ended = {}
    for k in range(1, 16):
        st = s.step(1)
        for b in (0, 1):
            if st[b] == "done" and b not in ended:
                ended[b] = k
    assert ended == {0: 6, 1: 8} and [s.n_gen(b) for b in (0, 1)] == [6, 8]
    s.rewind(0, 6, sampling=False)                                           # keep = n_gen: the ending is drawn again
    s.fork(3, 1, 8, 24, sampling=False)                                      # and in another slot, with a larger max_length
    s.fork(2, 1, 3, 24, sampling=False)
    again = {}
    for k in range(1, 8):
        st = s.step(1)
        for b in (0, 2, 3):
            if st[b] == "done" and b not in again:
                again[b] = k
    assert again == {0: 1, 3: 1, 2: 6}, "<eos> at the same step again"
    got = {b: s.take(b, return_logp=True) for b in (0, 1, 2, 3)}
    s.free()
    for b, text in ((0, Q[0]), (1, Q[1]), (2, Q[1]), (3, Q[1])):
        ref = alone(eng, ("Q", b), b, text, 16, False, 0)
        assert got[b][1] == ref[1] == (6 if b == 0 else 8) and torch.equal(got[b][0], ref[0]), b
        n = ref[1] + 1                                                       # the steps that ran: the tokens and the <eos> step
        assert torch.equal(got[b][2][:n], ref[2][:n]) and not got[b][2][n:].any(), b
        assert_b(eng, b, text, None, got[b], 0)


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_keep_zero_is_start_from():
    eng, A, c, spec = prompt0(3)

    def run(fork):
        s = eng.open_decode(S, max_positions=CAP)
        s.start(1, A, A.shape[0], STEPS, sampling=True, seed=11, continual=c)
        s.step(4)
        if fork:
            s.fork(0, 1, 0, 10, sampling=5, seed=7)
            s.fork(3, 1, 0, sampling=0.7, seed=9)
        else:
            s.start_from(0, 1, 10, sampling=5, seed=7)
            s.start_from(3, 1, sampling=0.7, seed=9)
        r = run_to_end(s, [0, 1, 3])
        s.free()
        return r

    a, b = run(True), run(False)
    assert all(same(a[i], b[i]) for i in (0, 1, 3)) and a[0][2].shape[0] == 10
    # in place: back to the prompt, the first sample drawn again from the prefix logits the slot kept
    s = eng.open_decode(S, max_positions=CAP)
    s.start(2, A, A.shape[0], STEPS, sampling=True, seed=11, continual=c)
    s.step(5)
    s.rewind(2, 0, sampling=5, seed=7)
    got = run_to_end(s, [2])[2]
    s.free()
    assert same(got, alone(eng, ("A", 3), 2, A, STEPS, 5, 7, c))


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_chains():
    eng, A, c, spec = prompt0(4)
    key = ("A", 4)
    s = eng.open_decode(S, max_positions=CAP)
    s.start(1, A, A.shape[0], STEPS, sampling=True, seed=11, continual=c)
    s.step(4)                                                                # 5 tokens
    s.fork(0, 1, 3, sampling=True, seed=11)
    s.step(3)                                                                # slot 0: 6 tokens
    s.fork(3, 0, 5, sampling=True, seed=11)                                  # a fork from a fork
    s.start_from(2, 0, sampling=5, seed=3)                                   # the prefix logits travelled with the fork
    got = run_to_end(s, [0, 1, 2, 3])
    s.start(1, A, A.shape[0], STEPS, sampling=True, seed=11, continual=c)
    s.step(2)
    s.start_from(0, 1, sampling=True, seed=4)
    s.step(3)
    s.fork(3, 0, 2, sampling=0.7, seed=5)                                    # a fork from a slot that was started from a slot
    s.step(1)
    s.start_from(2, 3, sampling=False)                                       # and a start_from from that
    got2 = run_to_end(s, [0, 1, 2, 3])
    s.free()
    ref = alone(eng, key, 1, A, STEPS, True, 11, c)
    assert same(got[0], ref) and same(got[1], ref) and same(got[3], ref)
    assert same(got[2], alone(eng, key, 2, A, STEPS, 5, 3, c))
    r0 = alone(eng, key, 0, A, STEPS, True, 4, c)
    assert same(got2[0], r0) and same(got2[1], ref)
    assert torch.equal(got2[3][0][: 4 + 2], r0[0][: 4 + 2]) and torch.equal(got2[3][2][:2], r0[2][:2])
    assert_b(eng, 3, A, c, got2[3], 4)
    assert same(got2[2], alone(eng, key, 2, A, STEPS, False, 0, c))


def test_a_fork_among_a_crowd():
    eng, P, spec = prompts(B3)
    Q = texts_of(EOS)
    A = P[0]
    s = eng.open_decode(S, max_positions=CAP)
    s.start(0, P[1], P[1].shape[0], 30, sampling=True, seed=5)               # one starts before the source
    s.step(2)
    s.start(1, A, A.shape[0], STEPS, sampling=True, seed=11)
    s.step(3)
    s.fork(2, 1, 2, sampling=True, seed=11)
    s.start(3, P[2], P[2].shape[0], 3, sampling=7, seed=11)                  # max_length 3: ends while the destination runs
    s.step(3)
    s.start(0, Q[0], Q[0].shape[0], 30, sampling=0.8, seed=3)                # the running slot 0 is abandoned for another prompt
    st = s.step(1)
    assert st[3] == "done", st
    s.take(3)
    s.fork(3, 2, 4, sampling=5, seed=2)                                      # a taken slot is the next destination
    s.step(1)
    s.start(0, Q[1], Q[1].shape[0], 30, sampling=True, seed=8)
    got = run_to_end(s, [1, 2, 3])
    s.free()
    ref = alone(eng, ("A", 0), 1, A, STEPS, True, 11)
    assert same(got[1], ref)
    assert same(got[2], ref), "the destination among unrelated slots that start, end, restart"
    assert torch.equal(got[3][0][:4], ref[0][:4]) and torch.equal(got[3][2][:4], ref[2][:4])
    assert_b(eng, 3, A, None, got[3], 0)


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_rules_refuse_before_anything_changes():
    from funcodec_amd.engine import EngineError
    eng, P, spec = prompts(B3)
    A = P[0]                                                                 # 7 text tokens: P = 9

    def session(with_refusals):
        s = eng.open_decode(S, max_positions=32)
        s.start(1, A, A.shape[0], 10, sampling=True, seed=21)                # the source
        s.start(3, P[1], P[1].shape[0], 10, sampling=0.7, seed=2)            # a bystander
        s.start(2, P[2], P[2].shape[0], 2, sampling=False)
        st = s.step(3)
        assert st[2] == "done" and s.n_gen(1) == 4, st
        s.take(2)                                                            # slot 2: free;  slot 0: never started
        if with_refusals:
            with pytest.raises(EngineError, match="slot 2"):
                s.fork(0, 2, 1)                                              # a free source
            with pytest.raises(EngineError, match="slot 0"):
                s.fork(2, 0, 1)                                              # a never-started source
            with pytest.raises(EngineError, match="slot 0"):
                s.rewind(0, 0)
            with pytest.raises(EngineError, match="slot 4"):
                s.fork(0, 4, 1)
            with pytest.raises(EngineError, match="slot -1"):
                s.fork(0, -1)
            with pytest.raises(EngineError, match="slot 4"):
                s.fork(4, 1, 1)
            with pytest.raises(EngineError, match=r"slot 0.*keep 5"):
                s.fork(0, 1, 5)                                              # the source has reported 4 tokens
            with pytest.raises(EngineError, match=r"slot 1.*keep 5"):
                s.rewind(1, 5)
            with pytest.raises(EngineError, match=r"slot 0.*max_length 3"):
                s.fork(0, 1, 3, 3)                                           # nothing left to generate
            with pytest.raises(EngineError, match=r"slot 1.*max_length 4"):
                s.rewind(1, 4, 4)
            with pytest.raises(EngineError, match=r"slot 0.*max_positions 32"):
                s.fork(0, 1, 2, 32 - 9 + 1)                                  # one position too many
            with pytest.raises(EngineError, match=r"slot 3.*max_positions 32"):
                s.fork(3, 1, 2, 40)                                          # the RUNNING bystander as destination: it must go on
            with pytest.raises(EngineError, match=r"slot 1.*max_positions 32"):
                s.rewind(1, 2, 40)                                           # the running source itself
            with pytest.raises(EngineError, match="top-k"):
                s.fork(0, 1, 2, sampling=0)
            with pytest.raises(EngineError, match="nucleus"):
                s.rewind(3, 1, sampling=0.0)
        r = run_to_end(s, [1, 3])
        s.free()
        return r

    a, b = session(True), session(False)
    assert same(a[1], b[1]) and same(a[3], b[3])
    # a failed slot is no source; a slot that ended by length cannot be kept whole without room to go on
    s = eng.open_decode(S, max_positions=32)
    s.start(1, A, A.shape[0], 4, sampling=False)
    step_until_done(s, [1])
    with pytest.raises(EngineError, match=r"slot 1.*max_length 4"):
        s.rewind(1, 4)
    with pytest.raises(EngineError, match=r"slot 0.*max_length 4"):
        s.fork(0, 1)
    s.fork(0, 1, None, 32 - 9, sampling=False)                               # exactly max_positions: accepted
    got = run_to_end(s, [0, 1])
    s.free()
    assert got[1][1] == 4 and 4 < got[0][1] <= 23 and torch.equal(got[0][0][:4], got[1][0])


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_generate_many_with_one_retry(tmp_path, monkeypatch):
    from funcodec_amd.bin.text2audio_inference import Text2Audio
    from funcodec_amd.config import arch_from_config, recipe_config
    from funcodec_amd.laura import DecodeSlots, retry_seed
    from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config
    from funcodec_amd.synth import make_laura_state_dict, make_state_dict, write_checkpoint
    c = MAN["e2e"]["laura_e2e_tinyphn_ds320"]
    lcfg = laura_recipe_config(c["laura_config"])
    spec = laura_spec_from_config(lcfg)
    lsd = make_laura_state_dict(lcfg, c["laura_seed"])
    ccfg = recipe_config(c["codec_config"])
    csd = make_state_dict(arch_from_config(ccfg), c["codec_seed"])
    lsd["quantizer_codebook.embed"] = csd["quantizer.rq.model.embed"][: spec.num_quantizers].copy()
    lc, lp = write_checkpoint(str(tmp_path / "laura"), lcfg, lsd)
    cc, cp = write_checkpoint(str(tmp_path / "codec"), ccfg, csd)
    M = 6
    t2a = Text2Audio(config_file=lc, model_file=lp, device="cuda", text_emb_model=None, beam_size=1, sampling=True, continual=True,
                     codec_config_file=cc, codec_model_file=cp, tokenize_to_phone=False, exclude_prompt=True, max_length=M,
                     max_positions=256)
    words = c["text"].split(" ")
    texts = [" ".join(words[i: 4 + 2 * i]) for i in range(2)]
    seeds = [100, 101]
    rewinds = []

    def counted(self, slot, keep, *a, _f=DecodeSlots.rewind, **k):
        rewinds.append((slot, keep))
        return _f(self, slot, keep, *a, **k)
    monkeypatch.setattr(DecodeSlots, "rewind", counted)
    rets, codecs = t2a.generate_many(texts, slots=2, seeds=seeds, retries=1)
    assert rewinds and all(keep == M // 2 for _, keep in rewinds), "the tiny model ends by length: at least one second try"
    n_auto = len(rewinds)
    # the same session by hand: start both, step(1); a slot that ends with n_gen == max_length is rewound once to n_gen // 2
    m = t2a.model
    enc = [t2a._encode_texts([t]) for t in texts]
    s = m.open_decode(2, logp=False)
    for i in (0, 1):
        s.start(i, enc[i][0][0, : enc[i][1][0]], enc[i][1][0], M, True, seeds[i])
    tried, hand = {0: 0, 1: 0}, {}
    for _ in range(4 * M):
        st = s.step(1)
        for i in (0, 1):
            if i in hand or st.get(i) != "done":
                continue
            if s.n_gen(i) >= M and tried[i] < 1:
                tried[i] += 1
                s.rewind(i, s.n_gen(i) // 2, M, True, retry_seed(seeds[i], 1))
            else:
                hand[i] = s.take(i)
        if len(hand) == 2:
            break
    s.free()
    assert len(rewinds) - n_auto == sum(tried.values()) == n_auto
    for i in (0, 1):
        tok, n = hand[i]
        assert codecs[i].shape[1] == n and torch.equal(codecs[i][0], tok), i
        wav = m.syn_audio(tok[None], enc[i][0], torch.tensor(enc[i][1]), t2a.codec_model)
        assert torch.equal(rets[i]["gen"], wav), (i, float((rets[i]["gen"] - wav).abs().max()))
    # retries = 0 is the call without the argument
    del rewinds[:]
    r0, c0 = t2a.generate_many(texts, slots=2, seeds=seeds, retries=0)
    r1, c1 = t2a.generate_many(texts, slots=2, seeds=seeds)
    assert not rewinds
    for i in (0, 1):
        assert torch.equal(c0[i], c1[i]) and torch.equal(r0[i]["gen"], r1[i]["gen"]) and torch.equal(r0[i]["gen_only_lm"], r1[i]["gen_only_lm"])
    assert any(not torch.equal(codecs[i], c1[i]) for i in (0, 1)), "a second try with another seed changes the second half"
