"""Decoding session of the LauraTTS engine on the GPU (LauraEngine.open_decode -> DecodeSlots, Text2Audio.generate_many): prompts join
and leave a running batch.  What is pinned:

* a session of ONE slot is decode_codec on the prompt alone, bit for bit (tokens, length, per-step log-probabilities), in every
  sampling mode, with and without a continual prompt;
* a slot depends on nothing but its own prompt and parameters: alone, crowded, in another slot -- the same bits;
* a session of S slots against decode_codec on each prompt alone stands as an S-row call stands: greedy tokens and lengths equal,
  log-probabilities within 1e-5 (the bar of test_laura.py::test_decode_is_batch_independent_and_reproducible, same fixture, S = 3, 10 steps);
* <eos>, forced tokens (LOGP_TOL against the reference's golden), the rules, chain against persistent step (2e-5, the bar of
  test_persistent_step_equals_the_kernel_chain), the time-out path, generate_many.
"""
import numpy as np
import pytest
import torch

from helpers import golden

from test_laura import LOGP_TOL, MAN, case_inputs, laura_engine

pytestmark = pytest.mark.gpu

B3, EOS = "laura_tiny_b3", "laura_tiny_eos_b2"


def texts_of(name):
    """[text_outs [len, D] of every prompt of the fixture]: the golden's text_outs, as test_laura.py feeds them."""
    outs = torch.from_numpy(golden(name)["text_outs"])
    return [outs[b, : n] for b, n in enumerate(MAN["cases"][name]["text_lengths"])]


def prompts(name):
    """(engine of the fixture's checkpoint, its prompts, spec)"""
    spec = case_inputs(name)[2]
    return laura_engine(name).engine, texts_of(name), spec


def run_to_end(sess, slots, limit=64):
    """step(1) until none of `slots` is running; {slot: take(return_logp=True)}"""
    for _ in range(limit):
        st = sess.step(1)
        if all(st.get(s) != "running" for s in slots):
            break
    assert all(st.get(s) == "done" for s in slots), st
    return {s: sess.take(s, return_logp=True) for s in slots}


def same(a, b):
    return a[1] == b[1] and torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


def continual_for(spec, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.integers(0, spec.codebook_size, size=(n, spec.predict_nq)).astype(np.int64))


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cont", [False, True])
@pytest.mark.parametrize("sampling,seed", [(False, 0), (True, 1234), (5, 7), (0.7, 7)])
def test_one_slot_is_decode_codec_alone_bit_for_bit(sampling, seed, cont):
    eng, P, spec = prompts(B3)
    steps = 12
    sess = eng.open_decode(1, max_positions=64)
    for b, p in enumerate(P):
        c = continual_for(spec, 4 + b, 50 + b) if cont else None     # the fixture has no continual prompt: random prompt tokens of 4, 5, 6 frames
        t, n, lp = eng.decode_codec(p[None], [p.shape[0]], steps, sampling=sampling, seed=seed, return_logp=True,
                                    continual=None if c is None else c[None], continual_lengths=None if c is None else [c.shape[0]])
        sess.start(0, p, p.shape[0], steps, sampling=sampling, seed=seed, continual=c)
        got = run_to_end(sess, [0])[0]
        assert got[1] == n[0], (b, got[1], n)
        assert torch.equal(got[0], t[0, : n[0]]), b
        assert torch.equal(got[2], lp[0]), (b, float((got[2] - lp[0]).abs().max()))
    sess.free()


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling,seed", [(False, 0), (True, 99)])
def test_a_slot_depends_on_nothing_but_its_own_prompt(sampling, seed):
    eng, P, spec = prompts(B3)
    Q = texts_of(EOS)                        # same width: two more prompts for the crowd
    A, steps = P[0], 12

    def alone(slot):
        s = eng.open_decode(4, max_positions=64)
        s.start(slot, A, A.shape[0], steps, sampling=sampling, seed=seed)
        r = run_to_end(s, [slot])[slot]
        s.free()
        return r

    ref = alone(2)
    s = eng.open_decode(4, max_positions=64)
    s.start(0, P[1], P[1].shape[0], 30, sampling=True, seed=5)                 # one starts before A
    s.step(2)
    s.start(2, A, A.shape[0], steps, sampling=sampling, seed=seed)
    s.start(3, P[2], P[2].shape[0], 3, sampling=7, seed=11)                    # max_length 3: ends while A runs
    s.step(3)
    s.start(1, Q[0], Q[0].shape[0], 30, sampling=0.8, seed=3)                  # one starts three steps after A
    st = s.step(1)
    assert st[3] == "done", st
    t3 = s.take(3)
    assert t3[1] <= 3
    s.start(3, Q[1], Q[1].shape[0], 30, sampling=True, seed=8)                 # taken and restarted with a fourth prompt
    crowded = run_to_end(s, [2])[2]
    s.free()
    assert same(crowded, ref), "A among three other prompts that start, end and restart around it"
    assert same(alone(0), ref), "A in slot 0"


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stagger", [0, 2])
def test_slots_against_the_one_utterance_call(stagger):
    eng, P, spec = prompts(B3)
    steps = 10
    s = eng.open_decode(3, max_positions=64)
    for b, p in enumerate(P):
        s.start(b, p, p.shape[0], steps, sampling=False)
        if stagger:
            s.step(stagger)
    got = run_to_end(s, [0, 1, 2])
    s.free()
    for b, p in enumerate(P):
        t1, o1, l1 = eng.decode_codec(p[None], [p.shape[0]], steps, sampling=False, return_logp=True)
        err = float((got[b][2] - l1[0]).abs().max())
        print("slot", b, "stagger", stagger, "max |logp - alone|", err)
        assert got[b][1] == o1[0] and torch.equal(got[b][0], t1[0, : o1[0]]), b
        assert err < 1e-5, (b, err)


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_eos_ends_a_slot_and_frees_it():
    eng, P, spec = prompts(EOS)
    c = MAN["cases"][EOS]
    assert c["tokens"] == [6, 8] and c["steps"] == [7, 9] and c["max_length"] == 16
    s = eng.open_decode(2, max_positions=64)
    for b, p in enumerate(P):
        s.start(b, p, p.shape[0], 16, sampling=False)
    ended = {}
    for k in range(1, 16):                       # the start drew sample 1; step k draws sample k + 1
        st = s.step(1)
        for b in (0, 1):
            if st[b] == "done" and b not in ended:
                ended[b] = k + 1
    assert ended == {0: 7, 1: 9}, ended
    first = {b: s.take(b, return_logp=True) for b in (0, 1)}
    assert [first[b][1] for b in (0, 1)] == [6, 8]
    g = golden(EOS)
    for b in (0, 1):
        assert np.array_equal(first[b][0].cpu().numpy(), g[f"tokens_{b}"].astype(np.int64))
    # step(16) reports both done; then slot 0, which ended, takes the OTHER prompt and ends where that prompt ends
    for b, p in enumerate(P):
        s.start(b, p, p.shape[0], 16, sampling=False)
    assert s.step(16) == {0: "done", 1: "done"}
    keep1 = s.take(1, return_logp=True)
    s.take(0)
    s.start(1, P[1], P[1].shape[0], 16, sampling=False)
    s.step(7)                                    # slot 1 is in the middle of its utterance
    s.start(0, P[1], P[1].shape[0], 16, sampling=False)
    again = run_to_end(s, [0, 1], limit=20)
    s.free()
    assert again[0][1] == 8 and torch.equal(again[0][0], first[1][0])
    assert same(again[1], keep1) and same(keep1, first[1])


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_forced_tokens_against_the_reference_golden():
    eng, P, spec = prompts(B3)
    c = MAN["cases"][B3]
    g = golden(B3)
    nq, M = spec.predict_nq, c["max_length"]
    s = eng.open_decode(3, max_positions=64)
    for b, p in enumerate(P):
        forced = np.zeros((M, nq), np.int64)
        t = g[f"tokens_{b}"].astype(np.int64)
        forced[: t.shape[0]] = t
        s.start(b, p, p.shape[0], M, sampling=False, forced=torch.from_numpy(forced))
    got = run_to_end(s, [0, 1, 2])
    s.free()
    for b in range(3):
        ref_lp = torch.from_numpy(g[f"logp_{b}"])
        n = min(ref_lp.shape[0], g[f"tokens_{b}"].shape[0] + 1, M)
        err = float((got[b][2].cpu()[:n] - ref_lp[:n]).abs().max())
        print("slot", b, "forced step form, max |logp - golden|", err)
        assert err < LOGP_TOL, (b, err)


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_rules_refuse_before_anything_changes():
    from funcodec_amd.engine import EngineError
    eng, P, spec = prompts(B3)

    def session(with_refusals):
        s = eng.open_decode(2, max_positions=32)
        s.start(0, P[0], P[0].shape[0], 10, sampling=True, seed=21)
        s.step(3)
        if with_refusals:
            with pytest.raises(EngineError, match=r"slot 1.*max_positions 32"):
                s.start(1, P[1], P[1].shape[0], 32 - P[1].shape[0] - 1, sampling=False)        # one position too many
            with pytest.raises(EngineError, match=r"slot 0.*max_positions 32"):
                s.start(0, P[1], P[1].shape[0], 40, sampling=False)                            # the RUNNING slot: it must go on
            with pytest.raises(EngineError, match="slot 2"):
                s.start(2, P[1], P[1].shape[0], 5)
            with pytest.raises(EngineError, match="slot -1"):
                s.start(-1, P[1], P[1].shape[0], 5)
            with pytest.raises(EngineError, match="top-k"):
                s.start(1, P[1], P[1].shape[0], 5, sampling=0)
            with pytest.raises(EngineError, match="slot 0 has not ended"):
                s.take(0)
            with pytest.raises(EngineError, match="slot 1 has not ended"):
                s.take(1)
            with pytest.raises(EngineError, match="slot 5"):
                s.take(5)
        s.start(1, P[2], P[2].shape[0], 32 - P[2].shape[0] - 2, sampling=False)                # exactly max_positions: accepted
        r = run_to_end(s, [0, 1])
        assert s.step(4) == {}                                                                 # no running slot: returns at once
        s.free()
        return r

    a, b = session(True), session(False)
    assert same(a[0], b[0]) and same(a[1], b[1])
    with pytest.raises(EngineError, match=r"1 \.\. 16 slots"):
        eng.open_decode(17)
    with pytest.raises(EngineError, match="max_positions"):
        eng.open_decode(2, max_positions=eng.max_positions + 4)


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_chain_and_persistent_step_agree():
    eng, P, spec = prompts(B3)
    s = eng.open_decode(3, max_positions=64)

    def run():
        s.start(0, P[0], P[0].shape[0], 12, sampling=False)
        s.step(2)
        for b in (1, 2):
            s.start(b, P[b], P[b].shape[0], 12, sampling=False)
        return run_to_end(s, [0, 1, 2])

    assert eng.set_persistent_step(True)
    pers = run()
    try:
        assert not eng.set_persistent_step(False)
        chain = run()                            # the SAME session, now on the kernel chain
    finally:
        eng.set_persistent_step(True)
    back = run()
    s.free()
    for b in range(3):
        err = float((pers[b][2] - chain[b][2]).abs().max())
        print("slot", b, "max |persistent - chain|", err)
        assert pers[b][1] == chain[b][1] and torch.equal(pers[b][0], chain[b][0])
        assert err < 2e-5, (b, err)
        assert same(back[b], pers[b])            # and back on the persistent step: its bits again


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_a_timed_out_hand_off_fails_the_running_slots_loudly(monkeypatch):
    eng, P, spec = prompts(B3)
    assert eng.set_persistent_step(True)
    try:
        eng.set_persistent_step(False)
        c = eng.open_decode(2, max_positions=64)
        for b in (0, 1):
            c.start(b, P[b], P[b].shape[0], 8, sampling=True, seed=31 + b)
        chain = run_to_end(c, [0, 1])
        c.free()
    finally:
        assert eng.set_persistent_step(True)
    s = eng.open_decode(2, max_positions=64)
    for b in (0, 1):
        s.start(b, P[b], P[b].shape[0], 8, sampling=True, seed=31 + b)
    s.step(2)
    before = eng.persistent_step_fallbacks
    monkeypatch.setenv("FC_LAURA_PERSIST_TEST", "timeout")
    with pytest.warns(RuntimeWarning, match="timed out at a hand-off"):
        st = s.step(2)
    monkeypatch.delenv("FC_LAURA_PERSIST_TEST")
    assert st == {0: "failed", 1: "failed"}
    assert eng.persistent_step_fallbacks == before + 1
    from funcodec_amd.engine import EngineError
    with pytest.raises(EngineError, match="slot 0 failed"):
        s.take(0)
    for b in (0, 1):                             # start revives a slot; the session stays on the kernel chain
        s.start(b, P[b], P[b].shape[0], 8, sampling=True, seed=31 + b)
    again = run_to_end(s, [0, 1])
    s.free()
    assert eng.persistent_step_fallbacks == before + 1
    assert same(again[0], chain[0]) and same(again[1], chain[1])


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_generate_many_keeps_two_slots_full(tmp_path):
    from funcodec_amd.bin.text2audio_inference import Text2Audio
    from funcodec_amd.config import arch_from_config, recipe_config
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
                     codec_config_file=cc, codec_model_file=cp, tokenize_to_phone=False, exclude_prompt=True, max_length=14,
                     max_positions=256)
    words = c["text"].split(" ")
    texts = [" ".join(words[i % 3: 4 + i]) for i in range(5)]               # five prompts of different lengths
    seeds = [100 + i for i in range(5)]
    rets, codecs = t2a.generate_many(texts, slots=2, seeds=seeds)
    assert len(rets) == len(codecs) == 5
    m = t2a.model
    for i, text in enumerate(texts):
        outs, lens = t2a._encode_texts([text])
        s = m.open_decode(2, logp=False)
        s.start(0, outs[0], lens[0], 14, sampling=True, seed=seeds[i])
        tok, n = run_alone(s)
        s.free()
        assert codecs[i].shape[1] == n and torch.equal(codecs[i][0], tok), i
        wav = m.syn_audio(tok[None], outs, torch.tensor(lens), t2a.codec_model)
        assert torch.equal(rets[i]["gen"], wav), (i, float((rets[i]["gen"] - wav).abs().max()))


def run_alone(s):
    for _ in range(32):
        if s.step(1).get(0) != "running":
            break
    return s.take(0)
