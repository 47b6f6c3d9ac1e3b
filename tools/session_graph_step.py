"""Time a push of a streaming session and of a slot session enqueued eagerly (some 60 launches) and as one replayed HIP graph
(open_stream / open_slots with graph=True), and split each time into what the host spends until the call returns and the rest.

ss320 and ds320wn lock-step pushes and ss320 / ss320tfc slot pushes, B / S = 1, 8, 32; 1 and 25 frames per push; encode and decode.
Warm-up, then the median of 24 pushes, the device synchronised around every push; the eager and the graphed form alternate push by
push inside one process, clocks as found.  Per cell: us per push, and of it the us until the call returned (`host`).  Before a cell is
timed the two forms' results are asserted torch.equal.
  lock-step   the library call itself (fc_stream_encode / fc_stream_decode_codes) with the same pointers at every push, on a stream of
              its own: what the graph replaces and nothing else.  `wrap`: the wrapper's call for the same push (CodecStream.encode /
              decode), which in the graphed form adds the copies into and out of the session's fixed buffers.
  slots       the wrapper's call for one assembled push (StreamSlots._encode_call / _decode_call), the slots out of phase as in
              tools/slots_step.py: a third START, the others continue, one ends.
--eager-only [--tree DIR]: the eager lock-step pushes alone, with funcodec_amd imported from DIR: the same measurement on another
checkout (the parent commit), for the comparison that shows the path without graph replay unchanged.  No pass / fail bar.

    python tools/session_graph_step.py [--out profiles/session_graph_step.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUSHES, WARM = 24, 6


def timed(fn):
    """(us until fn returned, us until the device was idle)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) * 1e6, (time.perf_counter() - t0) * 1e6


def med(pairs):
    return statistics.median(p[0] for p in pairs), statistics.median(p[1] for p in pairs)


class RawStream:
    """fc_stream_* with fixed pointers on a stream of its own: a running utterance behind its first push"""

    def __init__(self, m, B, nf, decode, graph):
        from funcodec_amd.engine import _ptr
        self.m, self.lib, self.ptr, self.decode, self.nf, self.B = m, m.engine.lib, _ptr, decode, nf, B
        hop, nq, D = m.engine.hop_length, m.arch.num_quantizers, m.arch.dimension
        self.st = m.open_stream(B, max_chunk=max(100, nf) * hop)
        head = max(self.st.min_first_frames if decode else self.st.min_first_samples // hop, nf)
        dev = m.device
        self.stream = torch.cuda.Stream()
        self.ws = torch.empty(self.st._ws_bytes, dtype=torch.uint8, device=dev)
        if graph:
            m.engine._check(self.lib.fc_graphstream_set(self.st._h, 1))
            assert self.lib.fc_graphstream_enabled(self.st._h)
        g = torch.Generator().manual_seed(11)
        self.tok = torch.randint(0, m.arch.codebook_size, (B, head, nq), generator=g).to(dev)
        self.wav_in = (0.1 * torch.randn(B, m.engine.channels, head * hop, generator=g)).to(dev)
        self.codes = torch.empty(nq * B * head, dtype=torch.int64, device=dev)
        self.quant = torch.empty(B * head * D, device=dev)
        self.wav = torch.empty(B * m.engine.channels * head * hop, device=dev)
        self.hop, self.nq, self.D = hop, nq, D
        self.x, self.t = self.wav_in, self.tok
        torch.cuda.synchronize()                            # the buffers were filled on the default stream, the pushes run on self.stream
        self.push(head)
        self.x, self.t = self.wav_in[..., :nf * hop].contiguous(), self.tok[:, :nf].contiguous()      # the steady push's inputs: fixed from here on
        torch.cuda.synchronize()

    def push(self, n=None):
        n = n or self.nf
        eng, h, ws, st = self.m.engine, self.st._h, self.ws, C.c_void_p(self.stream.cuda_stream)
        if self.decode:
            eng._check(self.lib.fc_stream_decode_codes(h, self.ptr(self.t), n, 1, self.ptr(self.wav), None, self.ptr(ws), ws.numel(), st))
            return (self.wav[:self.B * self.m.engine.channels * n * self.hop],)
        nfr = C.c_int(0)
        eng._check(self.lib.fc_stream_encode(h, self.ptr(self.x), n * self.hop, 0, self.ptr(self.codes), self.ptr(self.quant), None, C.byref(nfr),
                                             self.ptr(ws), ws.numel(), st))
        return self.codes[:self.nq * self.B * n], self.quant[:self.B * n * self.D]


def wrapped_stream(m, B, nf, decode, graph):
    """the wrapper's push of one steady chunk: () -> outputs"""
    hop, nq = m.engine.hop_length, m.arch.num_quantizers
    st = m.open_stream(B, max_chunk=max(100, nf) * hop, **({"graph": True} if graph else {}))
    head = max(st.min_first_frames if decode else st.min_first_samples // hop, nf)
    g = torch.Generator().manual_seed(12)
    if decode:
        src = torch.randint(0, m.arch.codebook_size, (B, head, nq), generator=g).cuda()
        push = lambda n: (st.decode(src[:, :n]),)
    else:
        src = (0.1 * torch.randn(B, head * hop, generator=g)).cuda()
        push = lambda n: st.encode(src[:, :n * hop])
    push(head)
    return (lambda: push(nf)), st


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def alternate(forms):
    """forms: callables; WARM + PUSHES rounds, every form once per round; medians (host us, total us) per form"""
    times = [[] for _ in forms]
    for i in range(WARM + PUSHES):
        for k, fn in enumerate(forms):
            times[k].append(timed(fn))
    return [med(t[WARM:]) for t in times]


def stream_cell(m, B, nf, decode, eager_only):
    e = RawStream(m, B, nf, decode, False)
    if eager_only:
        (he, te), = alternate([e.push])
        return f"eager {te:8.0f} (host {he:6.0f})"
    g = RawStream(m, B, nf, decode, True)
    for _ in range(5):
        a, b = e.push(), g.push()
        torch.cuda.synchronize()
        assert same(a, b), "graphed lock-step push differs from the eager one"
    we, ste = wrapped_stream(m, B, nf, decode, False)
    wg, stg = wrapped_stream(m, B, nf, decode, True)
    for _ in range(5):
        assert same(we(), wg()), "graphed wrapper push differs from the eager one"
    (he, te), (hg, tg), (hwe, twe), (hwg, twg) = alternate([e.push, g.push, we, wg])
    n = g.st.graph_stats()
    assert n["fallbacks"] == 0 and n["replays"] >= PUSHES and stg.graph_stats()["replays"] >= PUSHES
    return (f"eager {te:8.0f} (host {he:6.0f}) | graphed {tg:8.0f} (host {hg:6.0f}) {te / tg:5.2f}x | wrap eager {twe:8.0f} (host {hwe:6.0f}) "
            f"graphed {twg:8.0f} (host {hwg:6.0f}) {twe / twg:5.2f}x")


def roles(S, i):
    from funcodec_amd.stream import FC_SLOT_FINAL, FC_SLOT_START
    out, ended = [], False
    for b in range(S):
        r = (b + i) % 3
        f = FC_SLOT_START if r == 0 else 0
        if r == 2 and not ended:
            f, ended = FC_SLOT_FINAL, True
        out.append(f)
    return out


def slots_cell(m, S, nf, decode, cached):
    from funcodec_amd.stream import FC_SLOT_FINAL, FC_SLOT_START
    hop, nq = m.engine.hop_length, m.arch.num_quantizers
    sts = []
    for graph in (False, True):
        kw = {"max_chunk": max(100, 2 * nf) * hop}
        if cached:
            kw["max_frames"] = max(32, nf) + 3 * nf + 16
        sts.append(m.open_slots(S, graph=graph, **kw))
    st = sts[0]
    first = max(st.min_first_frames if decode else st.min_first_samples // hop, nf)
    g = torch.Generator().manual_seed(13)
    if decode:
        src = torch.randint(0, m.arch.codebook_size, (S, first, nq), generator=g).cuda()
    else:
        src = (0.1 * torch.randn(S, first * hop, generator=g)).cuda()

    def rows_of(flags):
        rows = {}
        for b, f in enumerate(flags):
            n = first if f & FC_SLOT_START else nf
            rows[b] = (src[b, :n], f) if decode else (src[b:b + 1, :n * hop - (1 if f & FC_SLOT_FINAL else 0)], f)
        return rows
    calls = [(lambda rows, s=s: s._decode_call(rows, True, False)) if decode else (lambda rows, s=s: s._encode_call(rows, False)) for s in sts]
    flat = lambda out: [t for k in sorted(out) for t in out[k] if t is not None]
    outs = [flat(c(rows_of([FC_SLOT_START] * S))) for c in calls]
    assert same(*outs)
    times = [[], []]
    for i in range(1, WARM + PUSHES + 1):
        rows = rows_of(roles(S, i))
        if i <= WARM:
            assert same(*[flat(c(rows)) for c in calls]), "graphed slot push differs from the eager one"
        else:
            for k, c in enumerate(calls):
                times[k].append(timed(lambda: c(rows)))
    n = sts[1].graph_stats()
    assert n["fallbacks"] == 0 and n["replays"] > 0, n
    (he, te), (hg, tg) = med(times[0]), med(times[1])
    return f"eager {te:8.0f} (host {he:6.0f}) | graphed {tg:8.0f} (host {hg:6.0f}) {te / tg:5.2f}x   [{n['captures']} captures, {n['replays']} replays]"


def model(name):
    from funcodec_amd.config import arch_from_config, recipe_config
    from funcodec_amd.model import EncodecMI355X
    from funcodec_amd.synth import make_state_dict
    arch = arch_from_config(recipe_config(name))
    m = EncodecMI355X(arch, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(arch, 0).items()})
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--eager-only", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the checkout funcodec_amd is imported from")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    lines = [f"# {args.label}" if args.label else "# us per push: median of 24, synchronised around each; host = us until the call returned"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    for name in ("ss320", "ds320wn"):
        m = model(name)
        for B in (1, 8, 32):
            for nf in (1, 25):
                for decode in (False, True):
                    emit(f"{name:8s} lock-step B={B:2d} frames={nf:2d} {'decode' if decode else 'encode'} | " + stream_cell(m, B, nf, decode, args.eager_only))
        if name == "ss320" and not args.eager_only:
            for S in (1, 8, 32):
                for nf in (1, 25):
                    for decode in (False, True):
                        emit(f"{name:8s} slots     S={S:2d} frames={nf:2d} {'decode' if decode else 'encode'} | " + slots_cell(m, S, nf, decode, False))
        del m
    if not args.eager_only:
        m = model("ss320tfc")
        for S in (1, 8, 32):
            for nf in (1, 25):
                for decode in (False, True):
                    emit(f"ss320tfc slots     S={S:2d} frames={nf:2d} {'decode' if decode else 'encode'} | " + slots_cell(m, S, nf, decode, True))


if __name__ == "__main__":
    main()
