"""DecodeSlots.start_from on the GPU: a slot started from the prompt another slot holds -- a device copy of the source's prefix (its
first text_len + 2 + cont_len key / value positions and the logits its prefix pass ended with) instead of a prefix pass -- is, bit for
bit, the slot that ``start`` gives for the same prompt and parameters.  "Equal" is test_laura_slots_gpu.same (length, tokens and per-step
log-probabilities by torch.equal); the ``start`` it is compared with runs alone in a session of the same S = 4 (the key ranges per head
depend on S).  Prompt 0 of laura_tiny_b3 has 7 text tokens: prefix lengths 9 (no continual prompt), 12 and 13 (3 and 4 prompt tokens)
cover P % 4 != 0 and P % 4 == 0, i.e. K rows with and without tail columns [P, pad4(P))."""
import numpy as np
import pytest
import torch

from test_laura import MAN
from test_laura_slots_gpu import B3, EOS, continual_for, prompts, run_to_end, same, texts_of

pytestmark = pytest.mark.gpu

S, CAP, STEPS = 4, 64, 12
_alone = {}


def alone(eng, key, slot, text, steps, sampling, seed, cont=None, forced=None, memo=True):
    """``start`` of one prompt alone in a session of S slots, run to its end.  Computed once per `key` and parameters, never changed."""
    k = (key, slot, steps, sampling, seed, None if forced is None else forced.numpy().tobytes())
    if not memo or k not in _alone:
        s = eng.open_decode(S, max_positions=CAP)
        s.start(slot, text, text.shape[0], steps, sampling=sampling, seed=seed, continual=cont, forced=forced)
        r = run_to_end(s, [slot])[slot]
        s.free()
        if not memo:
            return r
        _alone[k] = r
    return _alone[k]


def prompt0(cont_len):
    eng, P, spec = prompts(B3)
    return eng, P[0], (continual_for(spec, cont_len, 60 + cont_len) if cont_len else None), spec


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cont_len", [0, 3, 4])
@pytest.mark.parametrize("below,above", [((False, 0), (True, 1234)), ((5, 7), (0.7, 9))])
def test_a_copy_is_a_start(below, above, cont_len):
    eng, A, c, spec = prompt0(cont_len)
    assert (A.shape[0] + 2 + cont_len) % 4 == (0 if cont_len == 3 else 1)
    key = ("A", cont_len)
    s = eng.open_decode(S, max_positions=CAP)
    s.start(1, A, A.shape[0], STEPS, sampling=True, seed=11, continual=c)
    s.start_from(0, 1, STEPS, sampling=below[0], seed=below[1])              # one below the source, one above
    s.start_from(3, 1, STEPS, sampling=above[0], seed=above[1])
    got = run_to_end(s, [0, 1, 3])
    s.free()
    for slot, (sampling, seed) in ((0, below), (3, above)):
        ref = alone(eng, key, slot, A, STEPS, sampling, seed, c)
        assert got[slot][1] == ref[1] and torch.equal(got[slot][0], ref[0]), (slot, sampling)
        assert torch.equal(got[slot][2], ref[2]), (slot, sampling, float((got[slot][2] - ref[2]).abs().max()))
        if c is not None:
            assert torch.equal(got[slot][0][:cont_len].cpu(), c), "the destination's token row starts with the source's prompt tokens"
    # the source, with two slots started from it, is the source alone
    assert same(got[1], alone(eng, key, 1, A, STEPS, True, 11, c))


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_late_join_from_a_running_an_ended_and_a_copied_source():
    eng, A, c, spec = prompt0(4)
    key = ("A", 4)
    s = eng.open_decode(S, max_positions=CAP)
    s.start(1, A, A.shape[0], 8, sampling=True, seed=11, continual=c)
    s.step(5)
    s.start_from(0, 1, STEPS, sampling=5, seed=3)                            # the source has run 5 steps
    st = s.step(2)
    assert st[1] == "done", st                                               # max_length 8: the start's sample and 7 steps
    s.start_from(3, 1, sampling=True, seed=4)                                # the source has ended and is not taken; its max_length
    s.start_from(2, 0, STEPS, sampling=0.7, seed=5)                          # chained: from a destination, itself 2 steps on
    got = run_to_end(s, [0, 1, 2, 3])
    s.free()
    assert same(got[1], alone(eng, key, 1, A, 8, True, 11, c))
    assert same(got[0], alone(eng, key, 0, A, STEPS, 5, 3, c)), "from a source in the middle of its utterance"
    assert got[3][2].shape[0] == 8 and same(got[3], alone(eng, key, 3, A, 8, True, 4, c)), "from an ended source"
    assert same(got[2], alone(eng, key, 2, A, STEPS, 0.7, 5, c)), "from a slot that was itself started from a slot"


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_a_copy_among_a_crowd():
    eng, P, spec = prompts(B3)
    Q = texts_of(EOS)
    A = P[0]
    s = eng.open_decode(S, max_positions=CAP)
    s.start(0, P[1], P[1].shape[0], 30, sampling=True, seed=5)               # one starts before the source
    s.step(2)
    s.start(1, A, A.shape[0], STEPS, sampling=True, seed=11)
    s.step(1)
    s.start_from(2, 1, STEPS, sampling=True, seed=99)
    s.start(3, P[2], P[2].shape[0], 3, sampling=7, seed=11)                  # max_length 3: ends while the destination runs
    s.step(3)
    s.start(0, Q[0], Q[0].shape[0], 30, sampling=0.8, seed=3)                # the running slot 0 is abandoned for another prompt
    st = s.step(1)
    assert st[3] == "done", st
    s.take(3)
    s.start(3, Q[1], Q[1].shape[0], 30, sampling=True, seed=8)               # taken and restarted
    got = run_to_end(s, [1, 2])
    s.free()
    assert same(got[2], alone(eng, ("A", 0), 2, A, STEPS, True, 99)), "the destination among unrelated slots that start, end, restart"
    assert same(got[1], alone(eng, ("A", 0), 1, A, STEPS, True, 11))


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_forced_tokens_belong_to_the_slot_that_passes_them():
    eng, A, c, spec = prompt0(3)
    key = ("A", 3)
    rng = np.random.Generator(np.random.PCG64(77))
    f_src = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(STEPS, spec.predict_nq)).astype(np.int64))
    f_dst = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(STEPS, spec.predict_nq)).astype(np.int64))
    s = eng.open_decode(S, max_positions=CAP)
    s.start(1, A, A.shape[0], STEPS, sampling=False, continual=c, forced=f_src)
    s.step(2)
    s.start_from(0, 1, STEPS, sampling=False, forced=f_dst)
    s.start_from(3, 1, STEPS, sampling=True, seed=21)                        # from a forced source, without forced=: samples freely
    got = run_to_end(s, [0, 1, 3])
    s.free()
    ref = alone(eng, key, 0, A, STEPS, False, 0, c, forced=f_dst)
    assert torch.equal(got[0][0][3:].cpu(), f_dst) and same(got[0], ref), float((got[0][2] - ref[2]).abs().max())
    assert same(got[3], alone(eng, key, 3, A, STEPS, True, 21, c)) and not torch.equal(got[3][0][3:].cpu(), f_src)
    assert same(got[1], alone(eng, key, 1, A, STEPS, False, 0, c, forced=f_src))


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_copy_equals_start_in_both_step_forms():
    eng, A, c, spec = prompt0(4)

    def both():
        s = eng.open_decode(S, max_positions=CAP)
        s.start(1, A, A.shape[0], STEPS, sampling=True, seed=11, continual=c)
        s.step(3)
        s.start_from(2, 1, STEPS, sampling=5, seed=7)
        got = run_to_end(s, [2])[2]
        s.free()
        return got, alone(eng, None, 2, A, STEPS, 5, 7, c, memo=False)

    assert eng.set_persistent_step(True)
    try:
        assert not eng.set_persistent_step(False)
        got, ref = both()
        assert same(got, ref), "kernel chain"
    finally:
        assert eng.set_persistent_step(True)
    got, ref = both()
    assert same(got, ref), "persistent step"


# 6 ---------------------------------------------------------------------------------------------------------------------------
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
        assert st[2] == "done", st
        s.take(2)                                                            # slot 2: free;  slot 0: never started
        if with_refusals:
            with pytest.raises(EngineError, match="slot 2"):
                s.start_from(0, 2, 5)
            with pytest.raises(EngineError, match="slot 0"):
                s.start_from(2, 0, 5)
            with pytest.raises(EngineError, match="slot 4"):
                s.start_from(0, 4, 5)
            with pytest.raises(EngineError, match="slot -1"):
                s.start_from(0, -1)
            with pytest.raises(EngineError, match="slot 4"):
                s.start_from(4, 1, 5)
            with pytest.raises(EngineError, match="slot 1"):
                s.start_from(1, 1, 5)
            with pytest.raises(EngineError, match=r"slot 0.*max_positions 32"):
                s.start_from(0, 1, 32 - 9 + 1)                               # one position too many
            with pytest.raises(EngineError, match=r"slot 3.*max_positions 32"):
                s.start_from(3, 1, 40)                                       # the RUNNING bystander as destination: it must go on
            with pytest.raises(EngineError, match="top-k"):
                s.start_from(0, 1, 5, sampling=0)
        r = run_to_end(s, [1, 3])
        s.free()
        return r

    a, b = session(True), session(False)
    assert same(a[1], b[1]) and same(a[3], b[3])
    s = eng.open_decode(S, max_positions=32)
    s.start(1, A, A.shape[0], 4, sampling=False)
    s.start_from(0, 1, 32 - 9, sampling=False)                               # exactly max_positions: accepted
    assert run_to_end(s, [0, 1])[0][1] <= 23
    s.free()


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_generate_many_three_samples_of_three_prompts_over_four_slots(tmp_path, monkeypatch):
    from funcodec_amd.bin.text2audio_inference import Text2Audio
    from funcodec_amd.config import arch_from_config, recipe_config
    from funcodec_amd.laura import DecodeSlots
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
    t2a = Text2Audio(config_file=lc, model_file=lp, device="cuda", text_emb_model=None, beam_size=1, sampling=True, continual=True,
                     codec_config_file=cc, codec_model_file=cp, tokenize_to_phone=False, exclude_prompt=True, max_length=12,
                     max_positions=256)
    words = c["text"].split(" ")
    texts = [" ".join(words[i: 4 + 2 * i]) for i in range(3)]                # three prompts of different lengths
    seeds = [[100 + 10 * i + k for k in range(3)] for i in range(3)]
    calls = {"start": 0, "start_from": 0}
    for name in calls:
        def counted(self, *a, _f=getattr(DecodeSlots, name), _n=name, **k):
            calls[_n] += 1
            return _f(self, *a, **k)
        monkeypatch.setattr(DecodeSlots, name, counted)
    rets, codecs = t2a.generate_many(texts, slots=4, seeds=seeds, samples=3)
    assert calls["start"] + calls["start_from"] == 9 and calls["start_from"] >= 2, calls
    assert len(rets) == len(codecs) == 3 and all(len(r) == 3 for r in rets) and all(len(r) == 3 for r in codecs)
    calls.update(start=0, start_from=0)
    flat_r, flat_c = t2a.generate_many([t for t in texts for _ in range(3)], slots=4, seeds=[v for row in seeds for v in row])
    assert calls == {"start": 9, "start_from": 0}
    for i in range(3):
        for k in range(3):
            assert torch.equal(codecs[i][k], flat_c[3 * i + k]), (i, k)
            for part in ("gen", "gen_only_lm"):
                assert torch.equal(rets[i][k][part], flat_r[3 * i + k][part]), (i, k, part)
    assert any(not torch.equal(codecs[0][0], codecs[0][k]) for k in (1, 2)), "three seeds of one prompt: different candidates"
