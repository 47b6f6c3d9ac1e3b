"""The two attention forms of the LauraTTS engine and the decoding-step block around the step form, per op: the float64 references, the
input recipes and the bars that tests/test_laura_attention_gpu.py holds the kernels to -- and, here, without a GPU, the proof that those
references mean what the reference model means and that the inputs can tell a wrong kernel from a right one.

References (torch float64, written by explicit index, no rel_shift):
  * full-sequence rel-pos attention: s[i][j] = ((q_i + u) . k_j + (q_i + v) . p_{i-j}) / sqrt(dk), p_r = linear_pos(pe(r)) with pe the
    reference's float32 sinusoid values (laura_oracle.sinusoid_table) taken as given; keys >= len masked, the causal mask with the
    bidirectional prefix block (j <= i, or i and j both below bidir); masked probabilities exactly 0;
  * step form: one query at `pos` against keys 0 .. pos of the caches in the engine's layouts (k [B, d, Tcap], v [B, Tcap, d]);
  * the combination of the step kernel's raw key-range partials (unnormalised context o_s, running max m_s, sum l_s):
    sum_s e^(m_s - M) o_s / sum_s e^(m_s - M) l_s, with m_s = -inf (an empty range) weighing exactly 0;
  * the whole step block: LayerNorm (eps 1e-12), QKV, cache scatter at pos, attention, linear_out + residual, feed-forward + residual.

Checked here:
  * convention: the restatement agrees with laura_oracle.Stack._context (float32, rel_shift) within 1e-5 on tinylaura's stacks at T = 37;
  * power: for every input recipe of the GPU file, three deliberately wrong references -- relative positions shifted by one, the
    pos_bias_v term dropped, the last key of a range dropped (full form: each row's last visible key) -- differ from the true one by at
    least 100 x the bar the GPU file asserts (POWER x bar()), wherever the shape leaves room for the mistake: T >= POWER_MIN_T in the full
    form, every step case (each holds rows with hundreds of keys).  q and k are scaled so that the scores have a standard deviation
    near 2: a flat softmax hides all three mistakes.  The planted recipes put a key that wins by more than 50 in score into every second
    query row only (the direction it wins along is taken out of the other rows' queries), so the same tensors hold saturated rows and
    rows that still see every mistake;
  * the generators are seeded by the case alone, so this file and the GPU file see the same tensors.

Bars (tests/test_conv_layers.py, tests/test_freq_stft.py): K32 = 12 x the max error of the same operation in torch float32 on the CPU
against float64 over the same region (the engine's MFMA order and expf are not torch's), not below FLOOR = 1e-6 x max(1, max |ref|),
never above CAP = 2e-5 x max(1, max |ref|) (test_every_linear_against_torch_cpu's bar for one Linear).  The float32 operation is the
oracle's _context for the full form and the index restatement run in float32 for the step form and the block.
"""
import functools
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from laura_oracle import Stack, rel_pos_emb, sinusoid_table

from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config
from funcodec_amd.synth import make_laura_state_dict

K32, FLOOR, CAP = 12.0, 1e-6, 2e-5
POWER = 100.0
POWER_MIN_T = 15
WEIGHT_SEED = 3
SIG_QK = 1.3                  # q and k of the full form: scores then have a standard deviation near 2 (asserted below)
SIG_KC = 2.4                  # cached keys of the step form, whose q is the block's own (LayerNorm + Linear of x: about 0.6)
PLANT_SCORE = 80.0            # the planted key's lead in score before the ordinary terms; the lead that remains is asserted > 50
WRONG = ("rel_shift", "no_bias_v", "drop_last")

PREFIX = {"text_encoder": "text_encoder", "codec_lm": "codec_lm.encoder", "codec_encoder": "codec_encoder"}
# (model, stack, causal): head dimension 64, 32, 64 causal, 32 causal
FULL_STACKS = [("tinylaura", "text_encoder", False), ("tinylaura", "codec_encoder", False), ("tinylaura", "codec_lm", True),
               ("tinylaura32", "codec_lm", True)]
FULL_T = (1, 3, 4, 15, 16, 17, 31, 33, 65, 127, 128)          # 128 = max_positions of the full-sequence engines
FULL_MAXPOS = 128
BIDIR = (0, 1, 5, 16, 17, "len")
PLANT_KEYS = ("0", "last", "15", "16")
PLANT_T = (17, 65, 128)

STEP_MAXPOS = 512
STEP_POS = (0, 1, 2, 3, 4, 5, 127, 128, 129, 255, 256, 300, 511)
STEP_NS = (1, 2, 3, 8)
STEP_B = (1, 3, 16, 17, 33, 64)
STEP_MODELS = ("tinylaura", "tinylaura32")                    # the LM at head dimension 64 and 32
STEP_PLANTS = ("first", "last", "p127", "p128")
STEP_PLANT_B = (3, 17)


def bar(ref64: torch.Tensor, err32: float) -> float:
    top = max(1.0, float(ref64.abs().max()))
    return min(max(K32 * err32, FLOOR * top), CAP * top)


def model_cfg(name: str) -> dict:
    """tinylaura as it is; tinylaura32: its LM at head dimension 32; tinylaura320: an LM of width 320 with 10 heads"""
    cfg = laura_recipe_config("tinylaura")
    lm = cfg["model_conf"]["codec_lm_conf"]
    if name == "tinylaura32":
        lm.update(head=4, layer=2)
    elif name == "tinylaura320":
        lm.update(att_unit=320, head=10, unit=320, layer=2)
    elif name != "tinylaura":
        raise KeyError(name)
    return cfg


@functools.lru_cache(maxsize=None)
def model(name: str):
    cfg = model_cfg(name)
    sd = make_laura_state_dict(cfg, WEIGHT_SEED)
    return cfg, laura_spec_from_config(cfg), sd


@functools.lru_cache(maxsize=None)
def block_params(name: str, stack: str, layer: int):
    """What the attention of one block needs beside q, k, v, and (for the LM) the block's other weights, as float32 torch tensors"""
    _, spec, sd = model(name)
    s = getattr(spec, stack)
    p = f"{PREFIX[stack]}.encoders.{layer}"
    t = lambda k: torch.from_numpy(sd[f"{p}.{k}"])
    prm = types.SimpleNamespace(H=s.heads, dk=s.d_model // s.heads, d=s.d_model, u=t("self_attn.pos_bias_u"), v=t("self_attn.pos_bias_v"),
                                wpos=t("self_attn.linear_pos.weight"))
    if stack == "codec_lm":
        n1, n2 = s.norm_names
        prm.wqkv = torch.cat([t(f"self_attn.linear_{k}.weight") for k in "qkv"])
        prm.bqkv = torch.cat([t(f"self_attn.linear_{k}.bias") for k in "qkv"])
        prm.wout, prm.bout = t("self_attn.linear_out.weight"), t("self_attn.linear_out.bias")
        prm.w1, prm.b1, prm.w2, prm.b2 = t("feed_forward.w_1.weight"), t("feed_forward.w_1.bias"), t("feed_forward.w_2.weight"), t("feed_forward.w_2.bias")
        prm.n1g, prm.n1b, prm.n2g, prm.n2b = t(f"{n1}.weight"), t(f"{n1}.bias"), t(f"{n2}.weight"), t(f"{n2}.bias")
    return prm


def rel_pos_rows(prm, n: int, dtype) -> torch.Tensor:
    """p_r = linear_pos(pe(r)) for r = -(n - 1) .. n - 1 as [2 n - 1, H, dk], row r + n - 1; pe(r) the reference's float32 values"""
    pos, neg = sinusoid_table(n, prm.d, +1.0), sinusoid_table(n, prm.d, -1.0)
    pe = torch.cat([torch.flip(neg[1:], [0]), pos], 0)
    return (pe.to(dtype) @ prm.wpos.to(dtype).T).view(2 * n - 1, prm.H, prm.dk)


def visible(L: int, causal: bool, bid: int) -> torch.Tensor:
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    if not causal:
        return torch.ones(L, L, dtype=torch.bool)
    return (j <= i) | ((i < bid) & (j < bid))


def attention_ref(qkv, lens, prm, causal=False, bidir=None, dtype=torch.float64, wrong=None, scores=False):
    """Full-sequence rel-pos attention by explicit index: qkv [B, T, 3 d] (q | k | v) -> ctx [B, T, d], rows >= lens[b] zero.
    wrong: one of WRONG.  scores=True: the per-utterance (scores [H, L, L], visible [L, L]) instead."""
    B, T, _ = qkv.shape
    H, dk = prm.H, prm.dk
    q, k, v = qkv.to(dtype).view(B, T, 3, H, dk).unbind(2)
    P = rel_pos_rows(prm, T, dtype)
    u = prm.u.to(dtype)
    bv = torch.zeros_like(u) if wrong == "no_bias_v" else prm.v.to(dtype)
    off = 1 if wrong == "rel_shift" else 0
    out = torch.zeros(B, T, H * dk, dtype=dtype)
    kept = []
    for b in range(B):
        L = int(lens[b])
        i = torch.arange(L)
        rel = (i[:, None] - i[None, :] + off).clamp(-(T - 1), T - 1) + T - 1
        ac = torch.einsum("ihd,jhd->hij", q[b, :L] + u, k[b, :L])
        bd = torch.einsum("ihd,ijhd->hij", q[b, :L] + bv, P[rel])
        s = (ac + bd) / math.sqrt(dk)
        vis = visible(L, causal, int(bidir[b]) if bidir is not None else 0)
        if wrong == "drop_last":            # each row's last visible key, where it is not the only one
            last = (vis.long() * (i[None, :] + 1)).argmax(1)
            vis = vis.clone()
            vis[i[vis.sum(1) > 1], last[vis.sum(1) > 1]] = False
        kept.append((s, vis))
        p = torch.softmax(s.masked_fill(~vis, -math.inf), -1)
        out[b, :L] = torch.einsum("hij,jhd->ihd", p, v[b, :L]).reshape(L, H * dk)
    return kept if scores else out


def oracle_context32(qkv, lens, prm, causal=False, bidir=None):
    """laura_oracle.Stack._context (float32, rel_shift, masked_fill) on the caller's q, k, v: the projections are the three selections of
    x = qkv, which a float32 matmul does exactly."""
    B, T, _ = qkv.shape
    d = prm.d
    eye, z = torch.eye(d), torch.zeros(d, d)
    sd = {"X.encoders.0.self_attn.linear_pos.weight": prm.wpos, "X.encoders.0.self_attn.pos_bias_u": prm.u,
          "X.encoders.0.self_attn.pos_bias_v": prm.v}
    for n, name in enumerate("qkv"):
        sd[f"X.encoders.0.self_attn.linear_{name}.weight"] = torch.cat([eye if m == n else z for m in range(3)], 1)
        sd[f"X.encoders.0.self_attn.linear_{name}.bias"] = torch.zeros(d)
    st = Stack(sd, "X", types.SimpleNamespace(heads=prm.H, d_model=d))
    mask = torch.zeros(B, T, T, dtype=torch.bool)
    for b in range(B):
        L = int(lens[b])
        mask[b, :L, :L] = visible(L, causal, int(bidir[b]) if bidir is not None else 0)
        mask[b, L:, :L] = True              # padded query rows: any keys, they are not compared
    with torch.no_grad():
        return st._context(0, qkv, rel_pos_emb(T, d), mask)


def rows_below(lens, T):
    return (torch.arange(T)[None, :] < torch.tensor([int(v) for v in lens])[:, None])


def max_err(a, b, rows=None) -> float:
    e = (a.double() - b.double()).abs()
    if rows is not None:
        e = e[rows]
    return float(e.max()) if e.numel() else 0.0


# ---- input recipes of the full-sequence form ----------------------------------------------------------------------------------------
def full_lens(T: int):
    return [T, 1, T // 2 + 1]


def bidir_of(value, lens):
    return [int(L) if value == "len" else min(int(value), int(L)) for L in lens]


def _unit_orthogonal(rng, u):
    """per head, a unit direction orthogonal to u [H, dk] (float64)"""
    g = torch.from_numpy(rng.standard_normal(tuple(u.shape)))
    g = g - (g * u).sum(-1, keepdim=True) / (u * u).sum(-1, keepdim=True) * u
    return g / g.norm(dim=-1, keepdim=True)


def full_inputs(mname: str, stack: str, T: int, plant=None):
    """qkv [3, T, 3 d] float32 and the lengths.  plant in PLANT_KEYS: key 0 / len - 1 / 15 / 16 of every utterance that has it wins by
    PLANT_SCORE in the EVEN query rows; its direction is taken out of every query row first."""
    prm = block_params(mname, stack, 0)
    lens = full_lens(T)
    si = [s[:2] for s in FULL_STACKS].index((mname, stack))
    rng = np.random.Generator(np.random.PCG64([11, si, T, 0 if plant is None else 1 + PLANT_KEYS.index(plant)]))
    H, dk = prm.H, prm.dk
    q = torch.from_numpy(rng.standard_normal((3, T, H, dk))) * SIG_QK
    k = torch.from_numpy(rng.standard_normal((3, T, H, dk))) * SIG_QK
    v = torch.from_numpy(rng.standard_normal((3, T, H, dk)))
    planted = []
    if plant is not None:
        g = _unit_orthogonal(rng, prm.u.double())
        A, big = 8.0, PLANT_SCORE * math.sqrt(dk) / 8.0
        for b, L in enumerate(lens):
            js = L - 1 if plant == "last" else int(plant)
            if js >= L:
                continue
            q[b] -= (q[b] * g).sum(-1, keepdim=True) * g
            q[b, 0::2] += A * g
            k[b, js] += (big - (k[b, js] * g).sum(-1, keepdim=True)) * g
            planted.append((b, js))
    qkv = torch.stack([q, k, v], 2).reshape(3, T, 3 * H * dk).float().contiguous()
    return qkv, lens, planted


# ---- step form -------------------------------------------------------------------------------------------------------------------
def key_range(n: int, NS: int, s: int):
    """keys [k0, k1) of range s among NS over n keys, as attn_step_kernel splits them (whole quads per range)"""
    chunk = ((n + NS - 1) // NS + 3) & ~3
    k0 = s * chunk
    return k0, max(k0, min(k0 + chunk, n))


def step_attention_ref(q, kc, vc, pos, prm, dtype=torch.float64, wrong=None, NS=1, scores=False):
    """One query per row at pos[b] against keys 0 .. pos[b]: q [B, d], kc [B, d, Tcap], vc [B, Tcap, d] -> ctx [B, d].
    wrong "drop_last": the last key of each of the NS key ranges (never a row's only key)."""
    B = q.shape[0]
    H, dk = prm.H, prm.dk
    u = prm.u.to(dtype)
    bv = torch.zeros_like(u) if wrong == "no_bias_v" else prm.v.to(dtype)
    off = 1 if wrong == "rel_shift" else 0
    nmax = max(int(p) for p in pos) + 2
    P = rel_pos_rows(prm, nmax, dtype)
    out = torch.zeros(B, H * dk, dtype=dtype)
    kept = []
    for b in range(B):
        p_, n = int(pos[b]), int(pos[b]) + 1
        qb = q[b].to(dtype).view(H, dk)
        K = kc[b, :, :n].to(dtype).T.reshape(n, H, dk)
        V = vc[b, :n].to(dtype).reshape(n, H, dk)
        j = torch.arange(n)
        rel = p_ - j + off + nmax - 1
        s = (torch.einsum("hd,jhd->hj", qb + u, K) + torch.einsum("hd,jhd->hj", qb + bv, P[rel])) / math.sqrt(dk)
        keep = torch.ones(n, dtype=torch.bool)
        if wrong == "drop_last" and n > 1:
            for r in range(NS):
                k0, k1 = key_range(n, NS, r)
                if k1 > k0:
                    keep[k1 - 1] = False
        kept.append(s)
        pr = torch.softmax(s.masked_fill(~keep[None, :], -math.inf), -1)
        out[b] = torch.einsum("hj,jhd->hd", pr, V).reshape(H * dk)
    return kept if scores else out


def combine_partials(part: torch.Tensor) -> torch.Tensor:
    """raw key-range partials [B, H, NS, dk + 2] (o | m | l) -> ctx [B, H dk] in float64"""
    part = part.double()
    dk = part.shape[-1] - 2
    o, m, l = part[..., :dk], part[..., dk], part[..., dk + 1]
    M = m.max(-1, keepdim=True).values
    w = torch.where(torch.isinf(m) & (m < 0), torch.zeros_like(m), torch.exp(m - M))
    ctx = (w[..., None] * o).sum(2) / (w * l).sum(2)[..., None]
    return ctx.reshape(part.shape[0], -1)


def split_partials(q, kc, vc, pos, prm, NS, dtype=torch.float64):
    """what the step kernel leaves per key range, restated: [B, H, NS, dk + 2]; an empty range is (0 .. 0, -inf, 0)"""
    B = q.shape[0]
    H, dk = prm.H, prm.dk
    sc = step_attention_ref(q, kc, vc, pos, prm, dtype, scores=True)
    part = torch.zeros(B, H, NS, dk + 2, dtype=dtype)
    for b in range(B):
        n = int(pos[b]) + 1
        V = vc[b, :n].to(dtype).reshape(n, H, dk)
        for r in range(NS):
            k0, k1 = key_range(n, NS, r)
            if k1 <= k0:
                part[b, :, r, dk] = -math.inf
                continue
            s = sc[b][:, k0:k1]
            m = s.max(-1).values
            e = torch.exp(s - m[:, None])
            part[b, :, r, :dk] = torch.einsum("hj,jhd->hd", e, V[k0:k1])
            part[b, :, r, dk], part[b, :, r, dk + 1] = m, e.sum(-1)
    return part


def step_block_ref(x, kc, vc, pos, prm, dtype=torch.float64, wrong=None, NS=1):
    """One LM block of the decoding step: (new x [B, d], q, k column, v column, both caches after the scatter, ctx)"""
    c = lambda t: t.to(dtype)
    d = prm.d
    xd = c(x)
    y = F.layer_norm(xd, (d,), c(prm.n1g), c(prm.n1b), 1e-12)
    qkv = F.linear(y, c(prm.wqkv), c(prm.bqkv))
    q, k, v = qkv[:, :d], qkv[:, d: 2 * d], qkv[:, 2 * d:]
    kc2, vc2 = c(kc).clone(), c(vc).clone()
    for b in range(x.shape[0]):
        kc2[b, :, int(pos[b])] = k[b]
        vc2[b, int(pos[b])] = v[b]
    ctx = step_attention_ref(q, kc2, vc2, pos, prm, dtype, wrong, NS)
    x1 = xd + F.linear(ctx, c(prm.wout), c(prm.bout))
    y2 = F.layer_norm(x1, (d,), c(prm.n2g), c(prm.n2b), 1e-12)
    x2 = x1 + F.linear(torch.relu(F.linear(y2, c(prm.w1), c(prm.b1))), c(prm.w2), c(prm.b2))
    return x2, q, k, v, kc2, vc2, ctx


def step_rounds(B: int) -> int:
    """a case of fewer rows than STEP_POS has values runs as many rounds as cover them all"""
    return 1 if B >= len(STEP_POS) else -(-len(STEP_POS) // B)


def step_inputs(mname: str, B: int, NS: int, rnd: int = 0, plant=None, Tcap: int = STEP_MAXPOS):
    """x [B, d], k_cache [B, d, Tcap], v_cache [B, Tcap, d] (zero at and behind pos), pos [B] for block 0 of the model's LM.
    pos: STEP_POS in a seeded order, round after round, then seeded draws.  plant in STEP_PLANTS: in the EVEN rows that have such a key,
    the first key of the last non-empty range / the last key of range 0 (where it is not the new key) / key 127 / 128 of a range 0
    longer than one 128-key pass is set along the row's own q + u (float64 on the host) to win by PLANT_SCORE."""
    prm = block_params(mname, "codec_lm", 0)
    d, H, dk = prm.d, prm.H, prm.dk
    tag = [13, ["tinylaura", "tinylaura32", "tinylaura320"].index(mname), B, NS, 0 if plant is None else 1 + STEP_PLANTS.index(plant)]
    rng = np.random.Generator(np.random.PCG64(tag))
    order = [STEP_POS[i] for i in rng.permutation(len(STEP_POS))]
    if plant in ("p127", "p128"):
        order = sorted(STEP_POS, reverse=True)                 # the long rows first: they are the ones with such a key
    pool = order + [STEP_POS[i] for i in rng.integers(0, len(STEP_POS), size=max(0, B * step_rounds(B) - len(order)))]
    pos = [min(p, Tcap - 1) for p in pool[rnd * B: rnd * B + B]]
    rng = np.random.Generator(np.random.PCG64(tag + [rnd]))
    x = torch.from_numpy(rng.standard_normal((B, d))).float()
    kc = torch.from_numpy(rng.standard_normal((B, d, Tcap)) * SIG_KC).float()
    vc = torch.from_numpy(rng.standard_normal((B, Tcap, d))).float()
    planted = []
    if plant is not None:
        q = step_block_ref(x, torch.zeros(B, d, 1), torch.zeros(B, 1, d), [0] * B, prm)[1].view(B, H, dk)
        for b in range(0, B, 2):
            n = pos[b] + 1
            k0, k1 = key_range(n, NS, 0)
            if plant == "first":
                js = max(key_range(n, NS, r)[0] for r in range(NS) if key_range(n, NS, r)[1] > key_range(n, NS, r)[0])
            elif plant == "last":
                js = k1 - 1
            else:
                js = k0 + int(plant[1:]) if k1 - k0 > 128 else n
            if js >= pos[b]:
                continue
            qu = q[b] + prm.u.double()
            kc[b, :, js] = (PLANT_SCORE * math.sqrt(dk) / (qu * qu).sum(-1, keepdim=True) * qu).reshape(d).float()
            planted.append((b, js))
    for b in range(B):
        kc[b, :, pos[b]:] = 0.0
        vc[b, pos[b]:] = 0.0
    return x, kc, vc, pos, planted


def step_cases():
    """(model, B, key ranges, planted recipe or None) of the step-attention grid"""
    out = [(m, B, NS, None) for m in STEP_MODELS for B in STEP_B for NS in STEP_NS]
    # a range of 8 holds at most 64 of 512 keys: no key 127 / 128 there; the last key of ONE range is the new key, which is the block's own
    out += [(m, B, NS, pl) for m in STEP_MODELS for B in STEP_PLANT_B for NS in STEP_NS for pl in STEP_PLANTS
            if not (NS == 8 and pl[0] == "p") and not (NS == 1 and pl == "last")]
    out += [("tinylaura320", B, NS, None) for B in (3, 16) for NS in (2, 8)]
    return out


def block_cases():
    """the grid thinned for the whole block: every row count at the engine's own key-range rule (None), the extremes at two; the
    width-320 LM at the row counts around its predicted failure (13 rows and more)"""
    out = [(m, B, None) for m in STEP_MODELS for B in STEP_B]
    out += [(m, B, NS) for m in STEP_MODELS for B in (3, 17) for NS in (1, 8)]
    out += [("tinylaura320", B, None) for B in (3, 12, 13, 16, 33)]
    return out


def engine_key_ranges(mname: str, B: int) -> int:
    H = block_params(mname, "codec_lm", 0).H
    return max(1, min(8, 256 // (B * H)))


# ==================================================================================================================================
def test_models_of_this_file_are_accepted_configurations():
    for name, (d, H) in {"tinylaura": (128, 2), "tinylaura32": (128, 4), "tinylaura320": (320, 10)}.items():
        s = model(name)[1].codec_lm
        assert (s.d_model, s.heads) == (d, H) and s.d_model // s.heads in (32, 64)
    assert [block_params(m, s, 0).dk for m, s, _ in FULL_STACKS] == [64, 32, 64, 32]


@pytest.mark.parametrize("mname,stack,causal", FULL_STACKS)
def test_restatement_agrees_with_the_oracles_context(mname, stack, causal):
    """the real stack's weights and its own projections at T = 37: _context (float32, rel_shift) against the index form on the same
    float32 q, k, v -- this pins i - j, the sign of the table and the masks to the reference's semantics"""
    _, spec, sd = model(mname)
    s = getattr(spec, stack)
    T, lens = 37, [37, 20]
    rng = np.random.Generator(np.random.PCG64(5))
    sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
    st = Stack(sdt, PREFIX[stack], s)
    for layer in range(s.layers):
        prm = block_params(mname, stack, layer)
        x = torch.from_numpy(rng.standard_normal((2, T, s.d_model)).astype(np.float32)) * 2.0
        pre = f"{PREFIX[stack]}.encoders.{layer}.self_attn"
        qkv = torch.cat([F.linear(x, sdt[f"{pre}.linear_{k}.weight"], sdt[f"{pre}.linear_{k}.bias"]) for k in "qkv"], -1)
        for bid in ([None] if not causal else [None, [0, 0], [9, 20], [37, 5]]):
            mask = torch.zeros(2, T, T, dtype=torch.bool)
            for b in range(2):
                mask[b, :, : lens[b]] = True
                if causal:
                    mask[b, : lens[b], : lens[b]] = visible(lens[b], True, bid[b] if bid else 0)
            with torch.no_grad():
                ref32 = st._context(layer, x, rel_pos_emb(T, s.d_model), mask)
            got = attention_ref(qkv, lens, prm, causal, bid)
            assert max_err(got, ref32, rows_below(lens, T)) < 1e-5, (layer, bid)
            # and the selection form the bars are measured with is that very function
            assert max_err(oracle_context32(qkv, lens, prm, causal, bid), ref32, rows_below(lens, T)) < 1e-6


def test_step_reference_is_the_last_row_of_the_full_reference():
    """the step form's index convention (relative position pos - j >= 0, keys 0 .. pos) against the causal full form's last row"""
    for mname in STEP_MODELS:
        prm = block_params(mname, "codec_lm", 0)
        T = 41
        qkv, _, _ = full_inputs(mname, "codec_lm", 33)
        qkv = torch.cat([qkv[:1], qkv[1:2]], 1)[:, :T].contiguous()
        full = attention_ref(qkv, [T], prm, causal=True)
        d = prm.d
        kc = qkv[:, :, d: 2 * d].transpose(1, 2).contiguous()
        vc = qkv[:, :, 2 * d:].contiguous()
        for pos in (0, 1, 16, T - 1):
            got = step_attention_ref(qkv[:, pos, :d], kc, vc, [pos], prm)
            assert max_err(got[0], full[0, pos]) < 1e-12


def test_partials_combine_to_the_unsplit_reference_with_empty_ranges():
    prm = block_params("tinylaura32", "codec_lm", 0)
    x, kc, vc, pos, _ = step_inputs("tinylaura32", 16, 8)
    assert 0 in pos and 511 in pos
    _, q, _, _, kc2, vc2, ctx = step_block_ref(x, kc, vc, pos, prm)
    for NS in STEP_NS:
        part = split_partials(q, kc2, vc2, pos, prm, NS)
        b0 = pos.index(0)
        if NS > 1:
            assert bool(torch.isinf(part[b0, :, 1:, prm.dk]).all()) and float(part[b0, :, 1:, prm.dk + 1].abs().max()) == 0.0
        got = combine_partials(part)
        assert bool(torch.isfinite(got).all()) and max_err(got, ctx) < 1e-12, NS
    # m = -inf with garbage in o and l of that range still weighs nothing
    part = split_partials(q, kc2, vc2, pos, prm, 8)
    part[pos.index(0), :, 1:, : prm.dk] = 7.0
    assert max_err(combine_partials(part), ctx) < 1e-12


def _score_stats(kept):
    vals = torch.cat([s[:, vis].reshape(-1) for s, vis in kept if vis.shape[0] >= 8])
    return float(vals.std())


@pytest.mark.parametrize("mname,stack,causal", FULL_STACKS)
def test_full_form_inputs_can_tell_a_wrong_kernel(mname, stack, causal):
    prm = block_params(mname, stack, 0)
    cases = [(T, None) for T in FULL_T] + [(T, pl) for T in PLANT_T for pl in PLANT_KEYS]
    worst = {w: math.inf for w in WRONG}
    for T, plant in cases:
        qkv, lens, planted = full_inputs(mname, stack, T, plant)
        rows = rows_below(lens, T)
        for bid_v in (BIDIR if causal else (None,)):
            bid = bidir_of(bid_v, lens) if causal else None
            ref = attention_ref(qkv, lens, prm, causal, bid)
            if plant is None and T >= 31 and bid_v in (None, 0):
                sd_ = _score_stats(attention_ref(qkv, lens, prm, causal, bid, scores=True))
                assert 1.5 < sd_ < 2.5, (T, sd_)
            if plant is not None and bid_v in (None, 0, "len"):
                kept = attention_ref(qkv, lens, prm, causal, bid, scores=True)
                n_dom = 0
                for b, js in planted:
                    s, vis = kept[b]
                    for i in range(0, lens[b], 2):
                        if not vis[i, js] or int(vis[i].sum()) < 2:
                            continue
                        others = s[:, i, :].masked_fill(~vis[i][None, :], -math.inf).clone()
                        others[:, js] = -math.inf
                        assert float((s[:, i, js] - others.max(-1).values).min()) > 50.0, (T, plant, b, i)
                        n_dom += 1
                assert n_dom > 0, (T, plant)
            if T < POWER_MIN_T:
                continue
            e32 = max_err(oracle_context32(qkv, lens, prm, causal, bid), ref, rows)
            tol = bar(ref, e32)
            assert e32 < CAP, (T, plant, bid_v, e32)           # torch float32 itself sits under the cap: the bar is not the cap by default
            for w in WRONG:
                diff = max_err(attention_ref(qkv, lens, prm, causal, bid, wrong=w), ref, rows)
                worst[w] = min(worst[w], diff / tol)
                assert diff >= POWER * tol, (T, plant, bid_v, w, diff, tol)
    print(mname, stack, "smallest |wrong - true| / bar:", {w: f"{v:.3g}" for w, v in worst.items()})


@pytest.mark.parametrize("mname", STEP_MODELS + ("tinylaura320",))
def test_step_form_inputs_can_tell_a_wrong_kernel(mname):
    prm = block_params(mname, "codec_lm", 0)
    worst = {w: math.inf for w in WRONG}
    stds = []
    for m, B, NS, plant in step_cases():
        if m != mname:
            continue
        refs, f32s, wrongs, nplanted = [], [], {w: [] for w in WRONG}, 0
        for rnd in range(step_rounds(B)):
            x, kc, vc, pos, planted = step_inputs(m, B, NS, rnd, plant)
            x2, q, _, _, kc2, vc2, ctx = step_block_ref(x, kc, vc, pos, prm)
            q32, kc32, vc32 = q.float(), kc2.float(), vc2.float()       # what the kernel is given: float32 q and caches
            ref = step_attention_ref(q32, kc32, vc32, pos, prm)
            refs.append(ref)
            f32s.append(step_attention_ref(q32, kc32, vc32, pos, prm, torch.float32))
            for w in WRONG:
                wrongs[w].append(step_attention_ref(q32, kc32, vc32, pos, prm, wrong=w, NS=NS))
            sc = step_attention_ref(q32, kc32, vc32, pos, prm, scores=True)
            if plant is None:
                stds += [float(s[:, :-1].std()) for s, p in zip(sc, pos) if p >= 127]      # the cached keys (the new key is the block's own)
            for b, js in planted:
                others = sc[b].clone()
                others[:, js] = -math.inf
                assert float((sc[b][:, js] - others.max(-1).values).min()) > 50.0, (m, B, NS, plant, b)
            nplanted += len(planted)
        assert plant is None or nplanted > 0, (m, B, NS, plant)
        ref = torch.cat(refs)
        tol = bar(ref, max_err(torch.cat(f32s), ref))
        for w in WRONG:
            diff = max_err(torch.cat(wrongs[w]), ref)
            worst[w] = min(worst[w], diff / tol)
            assert diff >= POWER * tol, (m, B, NS, plant, w, diff, tol)
    assert stds and 1.5 < float(np.mean(stds)) < 2.5, float(np.mean(stds))
    print(mname, "score std", float(np.mean(stds)), "smallest |wrong - true| / bar:", {w: f"{v:.3g}" for w, v in worst.items()})


def test_block_cases_cover_the_grid_and_the_predicted_failure():
    cases = block_cases()
    assert {B for m, B, NS in cases if m == "tinylaura32"} >= set(STEP_B)
    # launch_gemv's old refusal: rows * H * 8 floats of range weights against KS * 256 of reduction scratch, KS = 4 at K = 320
    assert 12 * 10 * 8 <= 4 * 256 < 13 * 10 * 8
    assert ("tinylaura320", 16, None) in cases and ("tinylaura320", 13, None) in cases
    for m, B, NS in cases:
        assert 1 <= (NS or engine_key_ranges(m, B)) <= 8
    assert engine_key_ranges("tinylaura", 3) == 8 and engine_key_ranges("tinylaura32", 17) == 3 and engine_key_ranges("tinylaura", 64) == 2
