"""Text2Audio.generate_many as a sequence of session calls, no device: a stand-in model hands out scripted stand-in sessions (in the
style of the pair in test_laura_start_many_host.py), every call the sessions, the model and the codec receive is logged with its
arguments, and the complete ordered log of each case -- with what the call returned -- equals tests/golden/generate_many_calls.json.
The fixture was recorded by ``python tests/test_generate_many_calls_host.py`` on the commit before generate_many was rebuilt around
``laura.CandidateRun``: whatever ties the options together has to make the same calls in the same order.  And ``CandidateRun.close``
after an open that failed at either session."""
import json
import os

import pytest
import torch

from funcodec_amd.bin.text2audio_inference import Text2Audio
from funcodec_amd.laura import SamplingRules

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_many_calls.json")
MAX_LENGTH, NQ = 10, 2


def steps_of(seed, keep=0):
    """The scripted length of a candidate: 3 .. 12 steps by its seed, so some reach MAX_LENGTH and end by length."""
    return max(keep + 1, min(MAX_LENGTH, 3 + (seed * 7 + seed // 5) % 10))


class Session:
    """A DecodeSlots stand-in, plain, holding or queued: a slot runs steps_of(seed) steps, its tokens name its prompt and its seed."""

    def __init__(self, log, name, slots, kw, fail):
        self.log, self.name, self.slots, self.fail = log, name, int(slots), fail
        self.source, self.scored = kw.get("source"), kw.get("score", False)
        self.prefix_passes, self.calls = 0, 0
        self.moves, self.blocks_hist = (3, {1: 4, 2: 6}) if kw.get("elastic") else (0, {})
        self.rows = {}                       # slot -> dict(prompt=(fill, cont_len), seed, n, target)
        self.waiting, self.running, self.retired, self.claimed, self.tickets = [], {}, [], 0, 0

    def begin(self, slot, prompt, seed, n=0):
        self.rows[slot] = dict(prompt=prompt, seed=seed, n=n, target=steps_of(seed, n))

    def result(self, row, scored):
        fill, cont = row["prompt"]
        out = (torch.full((cont + row["n"], NQ), fill * 1000 + row["seed"] % 997, dtype=torch.int64), cont + row["n"])
        return out + ((-float(1 + row["seed"] % 13), row["n"], row["n"] < MAX_LENGTH),) if scored else out

    def start(self, slot, text_outs, text_len, max_length, sampling, seed, continual=None, rules=None):
        cont = 0 if continual is None else int(continual.shape[0])
        self.log.append(["start", self.name, slot, float(text_outs[0, 0]), list(text_outs.shape), text_len, max_length, sampling, seed, cont,
                         repr(rules)])
        self.prefix_passes += 1
        self.begin(slot, (int(text_outs[0, 0]), cont), seed)

    def start_many(self, requests):
        entry = []
        for row, r in requests.items():
            cont = 0 if r["continual"] is None else int(r["continual"].shape[0])
            entry.append([row, float(r["text_outs"][0, 0]), list(r["text_outs"].shape), r["text_len"], cont,
                          {k: repr(v) for k, v in sorted(r.items()) if k not in ("text_outs", "text_len", "continual")}])
            self.begin(row, (int(r["text_outs"][0, 0]), cont), 0)
        self.log.append(["start_many", self.name, entry])
        self.prefix_passes += 1

    def start_from(self, dst, src, max_length, sampling, seed, rules=None, source=None):
        self.log.append(["start_from", self.name, dst, src, max_length, sampling, seed, repr(rules), None if source is None else source.name])
        self.begin(dst, (source or self).rows[src]["prompt"], seed)

    def rewind(self, slot, keep, max_length, sampling, seed, rules=None):
        self.log.append(["rewind", self.name, slot, keep, max_length, sampling, seed, repr(rules)])
        self.begin(slot, self.rows[slot]["prompt"], seed, keep)

    def submit(self, row, max_length, sampling, seed, rules=None):
        self.log.append(["submit", self.name, row, max_length, sampling, seed, repr(rules)])
        self.waiting.append((self.tickets, row, seed))
        self.tickets += 1
        return self.tickets - 1

    def slot_tickets(self):
        return dict(self.running)

    def step(self, n):
        self.log.append(["step", self.name, n])
        self.calls += 1
        if self.source is not None:          # queued: free slots claim the oldest tickets at the head of every step, ended ones retire
            for _ in range(n):
                for slot in range(self.slots):
                    if slot not in self.rows and self.waiting:
                        ticket, row, seed = self.waiting.pop(0)
                        self.begin(slot, self.source.rows[row]["prompt"], seed)
                        self.running[slot] = ticket
                        self.claimed += 1
                for slot in sorted(self.rows):
                    self.rows[slot]["n"] += 1
                    if self.rows[slot]["n"] >= self.rows[slot]["target"]:
                        self.retired.append((self.running.pop(slot),) + self.result(self.rows.pop(slot), True))
            return {}
        status = {}
        for slot in sorted(self.rows):
            row = self.rows[slot]
            row["n"] = min(row["target"], row["n"] + n)
            status[slot] = "done" if row["n"] >= row["target"] else "running"
            if self.fail == (self.calls, slot):
                status[slot] = "failed"
                del self.rows[slot]
        return status

    def collect(self):
        out, self.retired = self.retired, []
        self.log.append(["collect", self.name, [t[0] for t in out]])
        return [(t, tokens, n, score if self.scored else None) for t, tokens, n, score in out]

    def n_gen(self, slot):
        self.log.append(["n_gen", self.name, slot])
        return self.rows[slot]["n"]

    def take(self, slot, return_score=False):
        self.log.append(["take", self.name, slot, return_score])
        return self.result(self.rows.pop(slot), return_score)

    def free(self):
        self.log.append(["free", self.name])


class Model:
    predict_nq, device = NQ, "cpu"

    def __init__(self, log, fail):
        self.log, self.fail, self.opened, self.drawn = log, fail, 0, 0

    def _next_seed(self):
        self.drawn += 1
        return 200 + self.drawn

    def open_decode(self, n, **kw):
        name = f"s{self.opened}"
        self.opened += 1
        self.log.append(["open_decode", name, n, {k: (v.name if k == "source" else v) for k, v in sorted(kw.items())}])
        return Session(self.log, name, n, kw, self.fail)

    def encode(self, text_in, lens):
        """A prompt's text_outs carry its last word: the request's number."""
        out = torch.zeros((text_in.shape[0], text_in.shape[1], 4))
        for b, n in enumerate(lens.tolist()):
            out[b, :n] = float(text_in[b, n - 1])
        return out, None

    def cal_codec_emb_batch(self, text_outs, lens, tokens, out_lens):
        self.log.append(["codec_emb", [float(v) for v in text_outs[:, 0, 0]], list(lens), [int(v) for v in tokens[:, 0, 0]], list(out_lens)])
        return tokens.float().sum(-1, keepdim=True).expand(-1, -1, 4)


class Codec:
    def __init__(self, log):
        self.log = log

    def __call__(self, x, bit_width=None, run_mod=None):
        self.log.append(["codec", run_mod, list(x.shape)])
        if run_mod == "encode":              # [[codes [n_q, 1, T / 10]]]
            return [[torch.full((4, 1, x.shape[-1] // 10), 7, dtype=torch.int64)]]
        return None, None, x.float().sum(-1)[:, None], None


def record(slots=2, seeds=True, prompts=False, fail=None, **options):
    """The log of one generate_many call over 5 requests, and what it returned."""
    log = []
    t2a = Text2Audio.__new__(Text2Audio)
    t2a.model, t2a.codec_model = Model(log, fail), Codec(log)
    t2a.continual, t2a.exclude_prompt, t2a.max_length, t2a.sampling = True, True, MAX_LENGTH, 5
    t2a.text_emb_model = lambda text: (torch.tensor([[int(w) for w in text.split()]]), torch.tensor([len(text.split())]))
    n, N = 5, options.get("samples", 1)
    texts = [" ".join([str(i)] * (2 + i % 3)) for i in range(n)]
    if seeds:
        seeds = [100 + i for i in range(n)] if N == 1 else [[100 + i * N + k for k in range(N)] for i in range(n)]
    more = dict(prompt_texts=["9"] * n, prompt_audios=[torch.zeros(1, 10 * (1 + i % 3)) for i in range(n)]) if prompts else {}
    out = t2a.generate_many(texts, slots=slots, seeds=seeds or None, **more, **options)

    def digest(ret, codec):
        return [list(ret["gen"].shape), float(ret["gen"].sum()), float(ret["gen_only_lm"].sum()), list(codec.shape), int(codec.sum())]

    flat = lambda v: v if N == 1 or options.get("keep") == "best" else [x for row in v for x in row]
    log.append(["returned", [digest(r, c) for r, c in zip(flat(out[0]), flat(out[1]))], [list(c) for c in out[2]] if len(out) > 2 else None,
                t2a.last_prefix_passes, {k: (v if k == "moves" else {str(b): s for b, s in v.items()}) for k, v in t2a.last_elastic.items()}
                if hasattr(t2a, "last_elastic") else None])
    return log


CASES = {
    "plain": dict(),
    "samples3": dict(samples=3),
    "samples2_retries1": dict(samples=2, retries=1),
    "samples3_best": dict(samples=3, keep="best"),
    "samples2_retries1_best": dict(samples=2, retries=1, keep="best"),
    "prefill4": dict(prefill=4),
    "prefill4_samples3": dict(prefill=4, samples=3),
    "prefill4_queue": dict(prefill=4, queue=True),
    "prefill4_queue_samples3_best": dict(prefill=4, queue=True, samples=3, keep="best"),
    "rules_drawn_seeds": dict(rules=SamplingRules(temperature=0.8, min_length=2), seeds=False),
    "rules_samples2_retries1": dict(rules=SamplingRules(temperature=0.8, min_length=2), samples=2, retries=1),
    "continual": dict(prompts=True),
    "continual_prefill4": dict(prompts=True, prefill=4),
    "continual_prefill4_queue_samples3": dict(prompts=True, prefill=4, queue=True, samples=3),
    "slots20": dict(slots=20),
    "slots20_elastic": dict(slots=20, elastic=True),
    "failed_slot": dict(fail=(2, 1)),
    "failed_slot_prefill4_samples3": dict(fail=(3, 0), prefill=4, samples=3),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_generate_many_makes_the_recorded_calls_in_the_recorded_order(case):
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    got = json.loads(json.dumps(record(**CASES[case])))
    assert len(got) > 10 and any(e[0] == "take" or e[0] == "collect" for e in got)
    assert got == want


@pytest.mark.parametrize("queue", [False, True])
@pytest.mark.parametrize("fails", [1, 2])
def test_close_frees_what_a_failed_open_left(queue, fails):
    """The holding session comes first with a queue and second without; whichever open fails, close frees the other and may be
    called again."""
    from funcodec_amd.laura import CandidateRun
    log = []

    class Failing(Model):
        def open_decode(self, n, **kw):
            if self.opened == fails - 1:
                raise RuntimeError("no room")
            return Model.open_decode(self, n, **kw)

    run = CandidateRun(5, 2, list(range(10)), None, None)
    assert run.close() is None
    with pytest.raises(RuntimeError, match="no room"):
        run.open(Failing(log, None), 2, prefill=4, queue=queue)
    counts = run.close()
    main_opened = fails == 2 and not queue
    assert counts == (dict(prefix_passes={"main": 0, "held": 0}, elastic=None) if main_opened else None)
    assert [e[0] for e in log] == ["open_decode", "free"][: 2 * (fails - 1)] and run.close() is None


if __name__ == "__main__":
    print("{" + ",\n".join(f"{json.dumps(case)}: {json.dumps(record(**CASES[case]))}" for case in sorted(CASES)) + "}")
