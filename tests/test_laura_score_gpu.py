"""Scores of a decoding session on the GPU (open_decode(score=True), DecodeSlots.score / score_row / take(return_score=True),
generate_many(keep="best")).  term[j] of a slot is the log-probability of generated step j's picks, the sum over the groups of
log softmax(logits[group])[pick]; what is pinned:

1. the terms against the session's own per-step log-probability rows, recomputed in float64: per term nq x 1e-5, the project's bar per
   log-probability entry times the entries summed -- every sampling mode, with and without prompt tokens, the
   ending <eos> step (the golden's, and a forced one);
2. a term is ONE function of the step's logits and final picks: top-k, and its tokens forced in greedy and in softmax mode: equal bits;
3. a slot depends on itself only, and scores change no other bit of a session;
4. fork / rewind / start_from carry the score of the path, on the kernel chain and on the persistent step;
5. the rules;  6. generate_many(keep="best").
No tolerance anywhere but in 1.  Sizes and helpers are those of test_laura_fork_gpu.py / test_laura_start_from_gpu.py."""
import numpy as np
import pytest
import torch

from test_laura import MAN
from test_laura_fork_gpu import step_until_done
from test_laura_slots_gpu import B3, EOS, prompts, same, texts_of
from test_laura_start_from_gpu import CAP, S, STEPS, alone, prompt0

pytestmark = pytest.mark.gpu

MODES = [(False, 0), (True, 1234), (5, 7), (0.7, 9)]


def finish(s, slot, logp=True):
    """an ended slot's (take, score row [CAP], count, end, score()); the slot is taken"""
    row, count, end = s.score_row(slot)
    sc = s.score(slot)
    assert sc[1] == count and sc[2] == (end == 2) and sc[0] == float(row[:count].double().sum())
    assert not row[count:].any(), "nothing behind the terms written"
    got = s.take(slot, return_logp=True) if logp else s.take(slot)
    return got, row, count, end, sc


def scored_alone(eng, slot, text, steps, sampling, seed, cont=None, forced=None):
    """``start`` of one prompt alone in a scored session of S slots, run to its end"""
    s = eng.open_decode(S, max_positions=CAP, score=True)
    s.start(slot, text, text.shape[0], steps, sampling=sampling, seed=seed, continual=cont, forced=forced)
    step_until_done(s, [slot])
    r = finish(s, slot)
    s.free()
    return r


def terms64(logp, picks, spec):
    """float64 terms from log-probability rows [n, V] and picks [n, nq]: per-group log-softmax of the row's slice at the pick, summed"""
    nq, G = spec.predict_nq, spec.codebook_size + 1
    assert logp.shape[1] == nq * G
    lp = logp.double().cpu().reshape(-1, nq, G)
    ls = lp - torch.logsumexp(lp, dim=2, keepdim=True)
    return ls.gather(2, picks.cpu().long()[:, :, None])[:, :, 0].sum(1)


def check_terms(row, logp, picks, spec, what):
    n = picks.shape[0]
    ref = terms64(logp[:n], picks, spec)
    err = float((row[:n].double() - ref).abs().max())
    print(what, "steps", n, "max |term - float64|", err, "bar", spec.predict_nq * 1e-5)
    assert err < spec.predict_nq * 1e-5, (what, err)
    return err


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cont_len", [0, 3])
@pytest.mark.parametrize("sampling,seed", MODES)
def test_terms_against_the_log_probability_rows(sampling, seed, cont_len):
    eng, A, c, spec = prompt0(cont_len)
    got, row, count, end, sc = scored_alone(eng, 1, A, STEPS, sampling, seed, c)
    n_gen = got[1] - cont_len
    assert count == n_gen + (1 if end == 2 else 0) and 1 <= n_gen <= STEPS and (end == 2 or n_gen == STEPS)
    # every step that left a token; the picks of an ending <eos> step are not recorded: the next two tests check that term
    check_terms(row, got[2], got[0][cont_len:], spec, f"sampling {sampling} cont_len {cont_len}")
    assert bool((row[:count] < 0).all()) and bool(torch.isfinite(row[:count]).all())


def test_terms_of_the_goldens_eos_steps():
    eng, Q, spec = prompts(EOS)
    assert MAN["cases"][EOS]["tokens"] == [6, 8]
    nq, G, K = spec.predict_nq, spec.codebook_size + 1, spec.codebook_size
    for b in (0, 1):
        got, row, count, end, sc = scored_alone(eng, b, Q[b], 16, False, 0)
        n = got[1]
        assert end == 2 and count == n + 1 == (7, 9)[b] and sc == (float(row[:count].double().sum()), n + 1, True)
        # greedy: the ending step's picks are the groups' first maxima, one of them <eos>
        last = got[2][n].cpu().reshape(nq, G).argmax(1)
        assert bool((last == K).any())
        check_terms(row, got[2], torch.cat([got[0].cpu(), last[None]]), spec, f"golden eos prompt {b}")


def test_a_forced_eos_row_is_scored_with_all_its_picks():
    eng, A, c, spec = prompt0(3)
    nq, K = spec.predict_nq, spec.codebook_size
    rng = np.random.Generator(np.random.PCG64(5))
    f = torch.from_numpy(rng.integers(0, K, size=(STEPS, nq)).astype(np.int64))
    f[5, nq - 1] = K                                                         # step 5 ends the utterance; its other groups count too
    for sampling, seed in ((False, 0), (5, 7)):
        got, row, count, end, sc = scored_alone(eng, 2, A, STEPS, sampling, seed, c, forced=f)
        assert got[1] == 3 + 5 and end == 2 and count == 6 and torch.equal(got[0][3:].cpu(), f[:5])
        check_terms(row, got[2], f[:6], spec, f"forced eos, sampling {sampling}")


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_one_function_of_logits_and_picks():
    eng, A, c, spec = prompt0(3)
    nq, K = spec.predict_nq, spec.codebook_size
    src, row, count, end, _ = scored_alone(eng, 1, A, STEPS, 5, 7, c)
    n = src[1] - 3
    assert n >= 4
    f = torch.cat([src[0][3:].cpu(), torch.full((1, nq), K, dtype=torch.int64)])      # its tokens, then an <eos> row in every group
    g, g_row, g_count, g_end, _ = scored_alone(eng, 1, A, n + 1, False, 0, c, forced=f)
    m, m_row, m_count, m_end, _ = scored_alone(eng, 1, A, n + 1, True, 99, c, forced=f)
    assert torch.equal(g[0], src[0]) and torch.equal(m[0], src[0]) and (g_count, g_end, m_count, m_end) == (n + 1, 2, n + 1, 2)
    assert torch.equal(g[2][: n + 1], m[2][: n + 1]) and torch.equal(g[2][:n], src[2][:n]), "the replays see the source's logits"
    assert torch.equal(g_row, m_row), float((g_row - m_row).abs().max())
    assert torch.equal(g_row[:n], row[:n]), float((g_row[:n] - row[:n]).abs().max())
    assert bool((g_row[: n + 1] != 0).all())


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling,seed", [(False, 0), (True, 99)])
def test_a_slot_depends_on_itself_only_and_scores_change_no_other_bit(sampling, seed):
    eng, P, spec = prompts(B3)
    Q = texts_of(EOS)
    A = P[0]
    ref, ref_row, ref_count, ref_end, ref_sc = scored_alone(eng, 2, A, STEPS, sampling, seed)
    for a in (0, 3):
        o = [i for i in range(4) if i != a]
        s = eng.open_decode(S, max_positions=CAP, score=True)
        s.start(o[0], P[1], P[1].shape[0], 30, sampling=True, seed=5)          # one starts before A
        s.step(2)
        s.start(a, A, A.shape[0], STEPS, sampling=sampling, seed=seed)
        s.start(o[1], P[2], P[2].shape[0], 3, sampling=7, seed=11)             # max_length 3: ends while A runs
        s.step(3)
        s.start(o[2], Q[0], Q[0].shape[0], 30, sampling=0.8, seed=3)           # one starts three steps after A
        st = s.step(1)
        assert st[o[1]] == "done", st
        t = s.take(o[1], return_score=True)
        assert t[1] <= 3 and t[2][1] >= 1
        s.start(o[1], Q[1], Q[1].shape[0], 30, sampling=True, seed=8)          # taken and restarted with a fourth prompt
        step_until_done(s, [a])
        got, row, count, end, sc = finish(s, a)
        s.free()
        assert same(got, ref), a
        assert torch.equal(row, ref_row) and (count, end, sc) == (ref_count, ref_end, ref_sc), a
    # the same prompt in a session without scores: tokens and log-probabilities, bit for bit
    assert same(ref, alone(eng, ("A", 0), 2, A, STEPS, sampling, seed))


# 4 ---------------------------------------------------------------------------------------------------------------------------
def check_branches(cont_len):
    from funcodec_amd.engine import EngineError
    eng, A, c, spec = prompt0(cont_len)
    ref, ref_row, ref_count, ref_end, ref_sc = scored_alone(eng, 1, A, STEPS, True, 11, c)
    assert ref[1] - cont_len >= 7, "the source must still run after 6 steps"
    s = eng.open_decode(S, max_positions=CAP, score=True)
    s.start(1, A, A.shape[0], STEPS, sampling=True, seed=11, continual=c)
    assert s.step(6)[1] == "running" and s.n_gen(1) == 7
    mid, mid_count, mid_end = s.score_row(1)
    assert (mid_count, mid_end) == (7, 0) and torch.equal(mid[:7], ref_row[:7]) and not mid[7:].any()
    with pytest.raises(EngineError, match="slot 1 has not ended"):
        s.score(1)
    # (a) the source's own mode and seed: the source's row and (sum, count)
    for dst, keep in ((0, 7), (2, 4), (3, 1)):
        s.fork(dst, 1, keep, sampling=True, seed=11)
        row, count, end = s.score_row(dst)
        assert (count, end) == (keep, 0) and torch.equal(row[:keep], ref_row[:keep]) and not row[keep:].any(), (dst, keep)
    step_until_done(s, [0, 1, 2, 3])
    for dst in (0, 2, 3):
        got, row, count, end, sc = finish(s, dst)
        assert same(got, ref) and torch.equal(row, ref_row) and (count, end, sc) == (ref_count, ref_end, ref_sc), dst
    # rewind of the ended source, keep 4: nothing stale behind the kept terms before a step runs, then the same end again
    assert ref_count > 4 and bool(ref_row[4:ref_count].any())
    s.rewind(1, 4, sampling=True, seed=11)
    row, count, end = s.score_row(1)
    assert (count, end) == (4, 0) and torch.equal(row[:4], ref_row[:4]) and not row[4:].any()
    # (b) another mode and seed from keep on; start_from beside it
    s.fork(0, 1, 4, sampling=5, seed=3)
    s.start_from(3, 1, STEPS, sampling=0.7, seed=9)
    step_until_done(s, [0, 1, 3])
    got1, row1, count1, end1, sc1 = finish(s, 1)
    assert same(got1, ref) and torch.equal(row1, ref_row) and (count1, end1, sc1) == (ref_count, ref_end, ref_sc)
    other, o_row, o_count, o_end, o_sc = finish(s, 0)
    dest, d_row, d_count, d_end, d_sc = finish(s, 3)
    s.free()
    n = other[1] - cont_len
    assert torch.equal(o_row[:4], ref_row[:4]) and torch.equal(other[0][: cont_len + 4], ref[0][: cont_len + 4])
    rep, r_row, r_count, r_end, r_sc = scored_alone(eng, 0, A, n, False, 0, c, forced=other[0][cont_len:].cpu())
    assert torch.equal(rep[0], other[0]) and torch.equal(r_row[:n], o_row[:n]), float((r_row[:n] - o_row[:n]).abs().max())
    assert o_count == n + (1 if o_end == 2 else 0) and r_count == n
    st, st_row, st_count, st_end, st_sc = scored_alone(eng, 3, A, STEPS, 0.7, 9, c)
    assert same(dest, st) and torch.equal(d_row, st_row) and (d_count, d_end, d_sc) == (st_count, st_end, st_sc), "start_from is start"


@pytest.mark.parametrize("cont_len", [0, 3, 4])
@pytest.mark.parametrize("form", ["chain", "persistent"])
def test_branches_carry_the_score_of_the_path(form, cont_len):
    eng = prompts(B3)[0]
    assert eng.set_persistent_step(True)
    if form == "persistent":
        check_branches(cont_len)
        return
    try:
        assert not eng.set_persistent_step(False)
        check_branches(cont_len)
    finally:
        assert eng.set_persistent_step(True)


def test_rewind_after_an_end_by_length_leaves_no_stale_term():
    eng, A, c, spec = prompt0(4)
    s = eng.open_decode(S, max_positions=CAP, score=True)
    s.start(1, A, A.shape[0], 8, sampling=True, seed=11, continual=c)
    step_until_done(s, [1])
    first, count, end = s.score_row(1)
    assert s.n_gen(1) == 8 and (count, end) == (8, 1) and bool((first[:8] != 0).all()), "ends by length"
    s.rewind(1, 4, sampling=True, seed=12)
    row, count, end = s.score_row(1)
    assert (count, end) == (4, 0) and torch.equal(row[:4], first[:4]) and not row[4:].any(), "zeros until overwritten"
    s.step(1)
    row, count, end = s.score_row(1)
    assert count == 5 and row[4] != 0 and not row[5:].any()
    step_until_done(s, [1])
    got, row, count, end, sc = finish(s, 1)
    s.free()
    n = got[1] - 4
    rep, r_row, _, _, _ = scored_alone(eng, 1, A, n, False, 0, c, forced=got[0][4:].cpu())
    assert torch.equal(r_row[:n], row[:n])


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_rules():
    from funcodec_amd.engine import EngineError
    eng, P, spec = prompts(B3)

    def session(with_refusals):
        s = eng.open_decode(S, max_positions=CAP)                            # without scores
        s.start(1, P[0], P[0].shape[0], 4, sampling=False)
        s.start(3, P[1], P[1].shape[0], 10, sampling=0.7, seed=2)            # a bystander
        st = s.step(3)
        assert st[1] == "done", st
        if with_refusals:
            with pytest.raises(EngineError, match=r"slot 1.*without scores"):
                s.take(1, return_score=True)
            with pytest.raises(EngineError, match=r"slot 1.*without scores"):
                s.score(1)
            with pytest.raises(EngineError, match=r"slot 3.*without scores"):
                s.score_row(3)
        step_until_done(s, [3])
        r = {i: s.take(i, return_logp=True) for i in (1, 3)}                 # the refused take left slot 1 ended, not freed
        s.free()
        return r

    a, b = session(True), session(False)
    assert same(a[1], b[1]) and same(a[3], b[3])
    # with scores: a slot that holds nothing has no score, a running one no (sum, count)
    s = eng.open_decode(S, max_positions=CAP, logp=False, score=True)
    s.start(1, P[0], P[0].shape[0], 4, sampling=False)
    with pytest.raises(EngineError, match="slot 0 holds no utterance"):
        s.score_row(0)
    with pytest.raises(EngineError, match="slot 4 outside"):
        s.score(4)
    with pytest.raises(EngineError, match="slot 1 has not ended"):
        s.score(1)
    step_until_done(s, [1])
    tok, n, sc = s.take(1, return_score=True)
    assert n == 4 and sc[1:] == (4, False) and sc == s_score_by_hand(eng, P[0])
    with pytest.raises(EngineError, match="slot 1 holds no utterance"):
        s.score(1)                                                           # taken: free
    s.free()


def s_score_by_hand(eng, text):
    got, row, count, end, sc = scored_alone(eng, 1, text, 4, False, 0)
    return sc


# 6 ---------------------------------------------------------------------------------------------------------------------------
def tiny_t2a(tmp_path, max_length):
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
                     codec_config_file=cc, codec_model_file=cp, tokenize_to_phone=False, exclude_prompt=True, max_length=max_length,
                     max_positions=256)
    words = c["text"].split(" ")
    return t2a, words


def count_fine_predictor(t2a, monkeypatch):
    """utterances that reach the fine predictor (cal_codec_emb_batch rows), counted by a wrapper"""
    seen = []
    inner = t2a.model.cal_codec_emb_batch

    def counted(text, text_lengths, codec, codec_lengths):
        seen.append(len(text_lengths))
        return inner(text, text_lengths, codec, codec_lengths)
    monkeypatch.setattr(t2a.model, "cal_codec_emb_batch", counted)
    return seen


def test_generate_many_keeps_the_best_of_three(tmp_path, monkeypatch):
    from funcodec_amd.laura import pick_best
    t2a, words = tiny_t2a(tmp_path, 12)
    texts = [" ".join(words[i: 4 + 2 * i]) for i in range(3)]                # three prompts of different lengths
    seeds = [[100 + 10 * i + k for k in range(3)] for i in range(3)]
    seen = count_fine_predictor(t2a, monkeypatch)
    out_all = t2a.generate_many(texts, slots=4, seeds=seeds, samples=3)
    assert sum(seen) == 9
    assert len(out_all) == 2 and all(len(v) == 3 and all(len(r) == 3 for r in v) for v in out_all), "keep='all' is today's shape"
    again = t2a.generate_many(texts, slots=4, seeds=seeds, samples=3, keep="all")
    del seen[:]
    rets, codecs, choice = t2a.generate_many(texts, slots=4, seeds=seeds, samples=3, keep="best")
    assert sum(seen) == 3, "the fine predictor ran on the winners only"
    assert len(rets) == len(codecs) == len(choice) == 3
    # every candidate again, one at a time in a scored session: its tokens are the keep='all' run's, its score is what is ranked
    m = t2a.model
    s = m.open_decode(4, logp=False, score=True)
    for i in range(3):
        to, ln = t2a._encode_texts([texts[i]])
        scores = []
        for k in range(3):
            s.start(k, to[0, : ln[0]], ln[0], 12, True, seeds[i][k])
            step_until_done(s, [k])
            tok, n, sc = s.take(k, return_score=True)
            assert out_all[1][i][k].shape[1] == n and torch.equal(out_all[1][i][k][0], tok), (i, k)
            assert torch.equal(again[1][i][k], out_all[1][i][k])
            scores.append(sc)
        k = pick_best(scores)
        print("request", i, "scores", scores, "kept", k)
        assert choice[i] == (k, scores[k][0] / scores[k][1]), (i, choice[i], scores)
        assert torch.equal(codecs[i], out_all[1][i][k]), i
        for part in ("gen", "gen_only_lm"):
            assert torch.equal(rets[i][part], out_all[0][i][k][part]), (i, part)
    s.free()


def test_generate_many_keeps_the_best_after_one_retry(tmp_path):
    from funcodec_amd.laura import pick_best, retry_seed
    M = 6
    t2a, words = tiny_t2a(tmp_path, M)
    texts = [" ".join(words[i: 4 + 2 * i]) for i in range(2)]
    seeds = [[100, 101], [110, 111]]
    rets, codecs, choice = t2a.generate_many(texts, slots=4, seeds=seeds, samples=2, retries=1, keep="best")
    # the same session by hand: candidate c in slot c; a slot that ends with n_gen == max_length is rewound once to n_gen // 2
    m = t2a.model
    enc = [t2a._encode_texts([t]) for t in texts]
    s = m.open_decode(4, logp=False, score=True)
    flat = [v for row in seeds for v in row]
    for c in range(4):
        i = c // 2
        s.start(c, enc[i][0][0, : enc[i][1][0]], enc[i][1][0], M, True, flat[c])
    tried, hand = {c: 0 for c in range(4)}, {}
    for _ in range(4 * M):
        st = s.step(1)
        for c in range(4):
            if c in hand or st.get(c) != "done":
                continue
            if s.n_gen(c) >= M and tried[c] < 1:
                tried[c] += 1
                s.rewind(c, s.n_gen(c) // 2, M, True, retry_seed(flat[c], 1))
            else:
                hand[c] = s.take(c, return_score=True)
        if len(hand) == 4:
            break
    s.free()
    assert len(hand) == 4 and sum(tried.values()) >= 1, "the tiny model ends by length: at least one second try"
    for i in range(2):
        scores = [hand[2 * i + k][2] for k in range(2)]
        k = pick_best(scores)
        tok, n, sc = hand[2 * i + k]
        assert sc[1] == (n + 1 if sc[2] else n), "the score of a rewound candidate counts its whole final path"
        assert choice[i] == (k, sc[0] / sc[1]), (i, choice[i], scores)
        assert codecs[i].shape[1] == n and torch.equal(codecs[i][0], tok), i
        wav = m.syn_audio(tok[None], enc[i][0], torch.tensor(enc[i][1]), t2a.codec_model)
        assert torch.equal(rets[i]["gen"], wav), (i, float((rets[i]["gen"] - wav).abs().max()))
