"""Elastic decoding sessions of the LauraTTS engine on the GPU (LauraEngine.open_decode(elastic=True) -> ElasticSlots,
fc_laura_slots_set_elastic / _step_blocks / _move, Text2Audio.generate_many(elastic=True)): a step as wide as the slots in use, rows
compacted.  Every equality is torch.equal -- the feature has no tolerance: a cut step is the full step on its rows and a move copies
words.  What is pinned:

* an elastic session of 17 / 33 slots equals its non-elastic twin (tokens, lengths, log-probability rows, score rows), greedy and
  top-k with rules, driven by step(1) and by step(5), while ``blocks`` falls 2 -> 1 / 3 -> 2 -> 1 as the high rows end;
* ``move`` on a plain wide session: a running slot mid-utterance, an ended one taken from its new row, a forked one, three in one
  call; another prompt started in the vacated row does not reach the moved slot; a start_from from the moved slot is ``start`` on
  its prompt (the kept prefix logits moved);
* compaction end to end at 33 slots: rows move down, the step shrinks to one block, a later start lands in the lowest free row, every
  take is the twin's;
* every refusal names the slot and changes nothing; queued sessions refuse move and set_elastic; generate_many(elastic=True) gives the
  tokens and waveforms of elastic=False.

The vacated-row check starts a FINITE other prompt there, not NaN text embeddings: all-NaN logits leave the sampler's arg-max at its
initial out-of-range id, which the next-input embedding then uses as a codebook row -- a wild read, not something a test may run.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_laura import MAN
from test_laura_slots_gpu import B3, EOS, prompts, run_to_end, same, texts_of

pytestmark = pytest.mark.gpu


def drive(sess, slots, n, limit=64):
    """step(n) until none of `slots` runs; ({slot: (tokens, len, logp, score row, count, end)}, [blocks after every call])"""
    seq = []
    for _ in range(limit):
        st = sess.step(n)
        seq.append(sess.blocks)
        if all(st.get(s) != "running" for s in slots):
            break
    assert all(st.get(s) == "done" for s in slots), st
    out = {}
    for s in slots:
        row = sess.score_row(s)
        out[s] = sess.take(s, return_logp=True) + row
    return out, seq


def same_scored(a, b):
    return same(a, b) and torch.equal(a[3], b[3]) and a[4:] == b[4:]


def start_all(sess, reqs):
    """{slot: request} through start_many, 16 per prefix pass, in slot order"""
    order = sorted(reqs)
    for i in range(0, len(order), 16):
        sess.start_many({s: reqs[s] for s in order[i: i + 16]})


def lengths(S):
    """max_length per slot, 3 .. 12: the highest row ends first, then its column block, block 0 last"""
    if S == 17:
        return [4 + (7 * i) % 9 for i in range(16)] + [3]
    return [8 + i % 5 for i in range(16)] + [4 + i % 4 for i in range(16)] + [3]


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["greedy", "topk_rules"])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("S", [17, 33])
def test_an_elastic_session_is_its_non_elastic_twin(S, n, mode):
    from funcodec_amd.laura import SamplingRules
    eng, P, spec = prompts(B3)
    L = lengths(S)
    assert min(L) == 3 and max(L) == 12
    rules = None if mode == "greedy" else SamplingRules(temperature=0.8, min_length=2, top_p=0.9, repeat_window=4, repeat_count=2)
    reqs = {i: dict(text_outs=P[i % 3], text_len=P[i % 3].shape[0], max_length=L[i], sampling=False if mode == "greedy" else 5,
                    seed=100 + i, rules=rules) for i in range(S)}

    def run(**kw):
        s = eng.open_decode(S, max_positions=64, score=True, wide=True, **kw)
        start_all(s, reqs)
        out = drive(s, range(S), n)
        extra = (s.rows(), s.moves) if kw else None
        s.free()
        return out + (extra,)

    got, seq, (rows, moves) = run(elastic=True)
    ref, full, _ = run()
    print("S", S, "n", n, mode, "blocks per call", seq, "twin", full)
    for i in range(S):
        assert same_scored(got[i], ref[i]), (S, n, mode, i)
    nb = (S + 15) // 16
    assert set(full) == {nb}
    assert seq[0] == nb and seq[-1] == 1 and seq == sorted(seq, reverse=True), seq
    assert set(seq) == set(range(1, nb + 1)), seq
    assert rows == {} and moves == 0                 # every row was busy or held until the end: nothing to compact


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_move_on_a_plain_wide_session():
    eng, P, spec = prompts(B3)
    Q = texts_of(EOS)
    A, B, Cc = P

    def scenario(move):
        s = eng.open_decode(20, max_positions=64, score=True, wide=True)
        at = dict(run=16, short=17, fork=18, other=19)
        s.start(16, A, A.shape[0], 12, sampling=True, seed=7)
        s.start(17, B, B.shape[0], 3, sampling=5, seed=8)
        s.start(19, Cc, Cc.shape[0], 12, sampling=0.8, seed=9)
        st = s.step(4)
        assert st[17] == "done" and st[16] == "running", st
        s.fork(18, 16, 2, sampling=True, seed=5)
        s.step(1)
        if move:
            s.move([(16, 3)])                                           # a running slot, mid-utterance
            at["run"] = 3
            st = s.step(1)
            assert st.get(3) == "running" and 16 not in st, st
            s.move([(17, 2), (18, 1), (19, 0)])                         # three in one call: an ended slot, a forked one, a running one
            at.update(short=2, fork=1, other=0)
            assert s.moves == 4
            # the vacated rows get other prompts: nothing of them may reach the moved slots
            s.start(16, Q[0], Q[0].shape[0], 30, sampling=True, seed=77)
            s.start(18, Q[1], Q[1].shape[0], 30, sampling=0.8, seed=78)
            s.start_from(5, at["run"], 10, sampling=5, seed=9)          # the kept prefix logits moved with the slot
        else:
            s.step(1)
            s.start(5, A, A.shape[0], 10, sampling=5, seed=9)
        assert s.n_gen(at["run"]) == 7
        short = s.score_row(at["short"])
        short = s.take(at["short"], return_logp=True) + short          # taken from its new row
        names = ["run", "fork", "other"]
        out, _ = drive(s, [at[k] for k in names] + [5], 1)
        s.free()
        res = {k: out[at[k]] for k in names}
        res.update(short=short, from_moved=out[5])
        return res

    got, ref = scenario(True), scenario(False)
    assert ref["short"][1] <= 3 and ref["run"][1] > 6
    for k in ref:
        assert same_scored(got[k], ref[k]), k


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_compaction_end_to_end():
    eng, P, spec = prompts(B3)
    S = 33
    early, late = list(range(24)), list(range(24, 33))                   # block 0 and half of block 1 end first
    reqs = {i: dict(text_outs=P[i % 3], text_len=P[i % 3].shape[0], max_length=3 if i < 24 else 9 + i % 4, sampling=True, seed=300 + i)
            for i in range(S)}

    def run(**kw):
        s = eng.open_decode(S, max_positions=64, score=True, wide=True, **kw)
        start_all(s, reqs)
        out, _ = drive(s, early, 1)
        assert s.blocks == 3
        st = s.step(1)                                                   # 9 utterances run in rows 24 .. 32, rows 0 .. 23 are free
        assert all(st[i] == "running" for i in late), st
        seen = (s.blocks, s.moves, s.rows()) if kw else None
        s.start(0, P[1], P[1].shape[0], 8, sampling=5, seed=55)
        where = s.rows()[0] if kw else None
        # the session as a SOURCE: another session names slot 30 by the caller's number, wherever its row is by now
        other = eng.open_decode(2, max_positions=64)
        other.start_from(0, 30, 6, sampling=True, seed=5, source=s)
        other.start(1, P[30 % 3], P[30 % 3].shape[0], 6, sampling=True, seed=5)
        copied = run_to_end(other, [0, 1])
        other.free()
        assert same(copied[0], copied[1]), "start_from(source=) from a moved slot is start on its prompt"
        more, _ = drive(s, late + [0], 2)
        out.update({("late", i): more[i] for i in late + [0]})
        s.free()
        return out, seen, where

    got, (blocks, moves, rows), where = run(elastic=True)
    ref, _, _ = run()
    assert blocks == 1 and moves == 9, (blocks, moves)
    assert sorted(rows) == late and sorted(rows.values()) == list(range(9)), rows
    assert rows[32] == 0 and rows[24] == 8, rows                         # highest busy rows into lowest free rows
    assert where == 9, where                                             # a start takes the lowest free row
    assert ref[("late", 24)][1] > 4
    for k in ref:
        assert same_scored(got[k], ref[k]), k


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_slot_and_change_nothing():
    from funcodec_amd import _lib
    from funcodec_amd.engine import EngineError
    eng, P, spec = prompts(B3)
    lib = eng.lib
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)

    def session(with_refusals):
        s = eng.open_decode(20, max_positions=64, score=True, wide=True)
        s.start(16, P[0], P[0].shape[0], 10, sampling=True, seed=21)
        s.start(17, P[1], P[1].shape[0], 2, sampling=True, seed=22)
        st = s.step(3)
        assert st == {16: "running", 17: "done"}
        if with_refusals:
            for pairs, what in [([(20, 1)], "source slot 20 outside 0 .. 19"), ([(16, 20)], "slot 20 outside 0 .. 19"),
                                ([(-1, 1)], "source slot -1 outside"), ([(16, -2)], "slot -2 outside"),
                                ([(16, 1), (16, 2)], "source slot 16 is named twice"), ([(16, 1), (17, 1)], "slot 1 is named twice"),
                                ([(16, 1), (1, 2)], "source slot 1 is also a destination"), ([(16, 3), (17, 16)], "slot 16 is also a source"),
                                ([(16, 16)], "slot 16 is also a source"),
                                ([(5, 1)], r"source slot 5 holds no utterance \(free or never started\)"),
                                ([(16, 1), (4, 2)], "source slot 4 holds no utterance"),
                                ([(16, 17)], r"slot 17 is not free \(ended, not taken\)"), ([(17, 16)], r"slot 16 is not free \(running\)")]:
                with pytest.raises(EngineError, match="move: " + what):
                    s.move(pairs)
            with pytest.raises(EngineError, match="move: no moves"):
                s.move([])
            for n in (0, -3, 21):                                        # the library's own count check, past the binding's
                assert lib.fc_laura_slots_move(s._handle(), n, i32(16), i32(1), None) != 0
                assert f"1 .. 20 moves per call, got {n}" in _lib.last_error()
            assert s.moves == 0
            assert s.step(1) == {16: "running", 17: "done"}
        else:
            s.step(1)
        out, _ = drive(s, [16, 17], 1)
        s.free()
        return out

    got, ref = session(True), session(False)
    for k in ref:
        assert same_scored(got[k], ref[k]), k

    # a queued session is fed by its queue only, and its slots are claimed on the device
    held = eng.open_decode(4, max_positions=64, logp=False)
    q = eng.open_decode(4, max_positions=64, logp=False, queue=8, source=held)
    with pytest.raises(EngineError, match="move: a queued session"):
        q.move([(0, 1)])
    assert lib.fc_laura_slots_move(q._handle(), 1, i32(0), i32(1), None) != 0 and "move: a queued session" in _lib.last_error()
    assert lib.fc_laura_slots_set_elastic(q._handle(), 1) != 0 and "set_elastic: a queued session" in _lib.last_error()
    with pytest.raises(EngineError, match="elastic=True is refused with queue="):
        eng.open_decode(4, max_positions=64, logp=False, queue=8, source=held, elastic=True)
    q.free()
    held.free()
    # the table's own refusals: the caller's slot numbers
    e = eng.open_decode(20, max_positions=64, wide=True, elastic=True)
    with pytest.raises(EngineError, match="slot 20 outside 0 .. 19"):
        e.start(20, P[0], P[0].shape[0], 5)
    with pytest.raises(EngineError, match=r"slot 7.*max_positions 64"):
        e.start(7, P[0], P[0].shape[0], 100)
    with pytest.raises(EngineError, match="slot 3 holds no utterance"):
        e.take(3)
    assert e.rows() == {} and e.step(1) == {} and e.blocks == 0
    e.free()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def equal(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and np.array_equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(equal(x, y) for x, y in zip(a, b))
    return a == b


def test_generate_many_elastic_is_generate_many(tmp_path):
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
                     codec_config_file=cc, codec_model_file=cp, tokenize_to_phone=False, exclude_prompt=True, max_length=12,
                     max_positions=256)
    words = c["text"].split(" ")
    texts = [" ".join(words[i % 3: 4 + i % 5]) for i in range(5)]
    seeds = [100 + i for i in range(5)]
    with pytest.raises(ValueError, match="elastic=True is refused with queue=True"):
        t2a.generate_many(texts, slots=20, seeds=seeds, prefill=4, queue=True, elastic=True)
    wav_e, tok_e = t2a.generate_many(texts, slots=20, seeds=seeds, elastic=True)
    assert set(t2a.last_elastic["blocks"]) == {1}, t2a.last_elastic    # 5 requests in rows 0 .. 4 of a 20-slot session: one block
    wav, tok = t2a.generate_many(texts, slots=20, seeds=seeds)
    assert len(tok) == 5 and equal(tok_e, tok) and equal(wav_e, wav)
    seeds2 = [[200 + 2 * i, 201 + 2 * i] for i in range(5)]
    best_e = t2a.generate_many(texts, slots=20, seeds=seeds2, samples=2, keep="best", elastic=True)
    best = t2a.generate_many(texts, slots=20, seeds=seeds2, samples=2, keep="best")
    assert len(best) == 3 and equal(best_e, best)
