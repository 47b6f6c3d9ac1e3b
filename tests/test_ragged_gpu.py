"""Length-aware (ragged) batches on the GPU, through the C ABI (fc_*_ragged): row b of a batch with ``lengths`` equals what the
offline call returns for that row ALONE cut at its length; zeros behind; nothing outside the row reaches it.

Bars: those of test_gpu_parity.py::test_e2e_against_reference_golden (:35-84), restated in ``_check_row`` with the line cited; a
differing code frame counts as equal only with that test's margin proof (test_gpu_parity.py:754-792, imported)."""
import functools

import numpy as np
import pytest
import torch

from helpers import audio, engine_for, golden, index_report, manifest, oracle_for, rms, state_for
from test_gpu_parity import WAV_RMS_TOL, _assert_flips_are_near_ties, _prefix_before

pytestmark = pytest.mark.gpu
MAN = manifest()


def _fill(rows, Tmax, mode, seed=0):
    """Rows [C?, len] stacked into [B, (C,) Tmax]; behind a row's end: zeros, NaN, or the row wrapped around (what the CLI's
    pad_list_with_mod(..., "wrap") collation leaves there)."""
    out = []
    for x in rows:
        n = x.shape[-1]
        if mode == "wrap":
            reps = -(-Tmax // n)
            y = torch.cat([x] * reps, -1)[..., :Tmax]
        else:
            y = torch.full(x.shape[:-1] + (Tmax,), float("nan") if mode == "nan" else 0.0)
            y[..., :n] = x
        out.append(y)
    return torch.stack(out, 0).contiguous()


def _ref_from_golden(name, row):
    c, g = MAN["cases"][name], golden(name)
    wav = audio(c["batch"], c["samples"], c["audio_seed"], c["audio_kind"], c.get("channels", 1))[row]
    ref = dict(indices=g["indices"].astype(np.int64)[:, row:row + 1], quantized=g["quantized"][row:row + 1], recon=g["recon"][row:row + 1])
    for k in ("encoder_out", "scale", "recon_from_codes"):
        if k in g:
            ref[k] = g[k][row:row + 1]
    return wav, ref, name


@functools.lru_cache(maxsize=None)
def _seeded_row(cfg_name, seed, decay, n, s, ch, bw):
    """A seeded utterance of n samples and its one-utterance oracle result (computed once for the three fill modes)."""
    w = audio(1, n, 4000 + s, "noise" if s % 2 else "tones", ch)[0]
    return _ref_from_oracle(cfg_name, seed, decay, w, bw, f"{cfg_name}:oracle:{n}")


def _ref_from_oracle(cfg_name, seed, decay, wav, bw, tag):
    orc = oracle_for(cfg_name, seed, decay)
    o = orc.inference(wav[None], bit_width=bw, use_scale=True)
    emb, sc = o["code_embeddings"][0]
    ref = dict(indices=o["code_indices"][0].numpy().astype(np.int64), quantized=emb.numpy(), recon=o["recon_speech"].numpy(),
               encoder_out=o["encoder_out"].numpy())
    if sc is not None:
        ref["scale"] = sc.reshape(1, -1).numpy()
    return wav, ref, tag


def _check_row(m, sd, arch, tag, b, n, got, dec, ref):
    """One row against its one-utterance reference, with the bars of test_e2e_against_reference_golden."""
    hop = m.engine.hop_length
    Tf = m.engine.frames(n)
    assert ref["indices"].shape[2] == Tf, (tag, ref["indices"].shape, Tf)
    enc = got["enc_out"][b:b + 1, :Tf]
    if "encoder_out" in ref:
        assert rms(enc, ref["encoder_out"]) < 2e-5, tag                                           # test_gpu_parity.py:42
    if "scale" in ref:
        s_ref = torch.from_numpy(np.asarray(ref["scale"])).reshape(-1)
        assert float(((got["scale"][b].cpu().reshape(-1) - s_ref).abs() / s_ref).max()) < 1e-5, tag   # :44
    codes = got["codes"][:, b:b + 1, :Tf]
    rep = index_report(codes, ref["indices"])
    projected = arch.codebook_dim != arch.dimension
    qtol = 1e-5 * float(np.sqrt((ref["quantized"] ** 2).mean())) if projected else 0.0             # :53
    recon = got["recon"][b:b + 1, :, :n]
    print(f"{tag}: row {b} len {n}: {rep['frames_bad']} of {rep['frames']} frames differ")
    if rep["mismatched_indices"] == 0:
        assert rms(got["quantized"][b:b + 1, :Tf], ref["quantized"]) <= qtol, tag                  # :55
        assert rms(recon, ref["recon"]) < WAV_RMS_TOL, tag                                         # :56
    else:
        def qin(x):                                                                                # :59-63
            x = torch.as_tensor(x).float().cpu()
            if projected:
                x = torch.nn.functional.linear(x, torch.from_numpy(sd["quantizer.input_proj.weight"]), torch.from_numpy(sd["quantizer.input_proj.bias"]))
            return torch.tanh(x) * arch.codec_range if arch.codec_range else x
        proofs = _assert_flips_are_near_ties(sd["quantizer.rq.model.embed"], qin(ref["encoder_out"]), ref["indices"], codes, got_enc=qin(enc),
                                             max_frames=max(1, rep["frames"] // 250))              # :64-65
        cut = _prefix_before([p[1] for p in proofs], Tf, hop, 0)
        k = n if cut is None else min(cut, n)
        if k > 0:
            assert rms(recon[..., :k], np.asarray(ref["recon"])[..., :k]) < WAV_RMS_TOL, (tag, k)  # :68-72
    # decoded from the REFERENCE's codes / embeddings with token_lengths                             :74-84
    w2, emb, w3 = dec["w2"][b:b + 1], dec["emb"][b:b + 1, :Tf], dec["w3"][b:b + 1]
    assert rms(emb, ref["quantized"]) <= qtol, tag
    if "recon_from_codes" in ref:
        assert rms(w2[..., :Tf * hop], ref["recon_from_codes"]) < WAV_RMS_TOL, tag
        assert rms(w3[..., :Tf * hop], ref["recon_from_codes"]) < WAV_RMS_TOL, tag
    else:
        sc = torch.from_numpy(np.asarray(ref["scale"])).view(-1, 1, 1) if "scale" in ref else 1.0
        assert rms(w2.cpu()[..., :n] * sc, ref["recon"]) < WAV_RMS_TOL, tag
        assert rms(w3.cpu()[..., :n] * sc, ref["recon"]) < WAV_RMS_TOL, tag
    # tails: everything behind the row's valid part is exactly zero
    Tfm = got["codes"].shape[2]
    assert int(got["codes"][:, b, Tf:].abs().sum()) == 0 and float(got["quantized"][b, Tf:].abs().sum()) == 0.0, tag
    assert float(got["enc_out"][b, Tf:].abs().sum()) == 0.0 and float(got["sub_quants"][:, b, :, Tf:].abs().sum()) == 0.0, tag
    assert float(got["recon"][b, :, n:].abs().sum()) == 0.0, tag
    assert float(dec["w2"][b, :, Tf * hop:].abs().sum()) == 0.0 and float(dec["w3"][b, :, Tf * hop:].abs().sum()) == 0.0, tag
    assert float(dec["emb"][b, Tf:].abs().sum()) == 0.0 and Tfm >= Tf, tag


def _run(m, rows, n_q, mode):
    """rows: [(wav [C?, len], ref, tag)] -> the ragged calls' outputs for the batch, and the decodes of the references' codes / embeddings."""
    lens = [r[0].shape[-1] for r in rows]
    Tmax = max(lens)
    wav = _fill([r[0] for r in rows], Tmax, mode)
    L = torch.tensor(lens, dtype=torch.int32)
    e = m.engine
    got = e.encode(wav, n_q, want_enc_out=True, lengths=L)
    r2 = e.encode_decode(wav, n_q, use_scale=True, lengths=L)
    assert torch.equal(r2["codes"], got["codes"])
    assert torch.equal(r2["quantized"], got["quantized"])
    got["recon"] = r2["recon"]
    for v in got.values():
        assert v is None or bool(torch.isfinite(v.float()).all()), "a NaN behind len_b reached an output"
    Tfm, D = e.frames(Tmax), m.arch.dimension
    fl = torch.tensor([e.frames(n) for n in lens], dtype=torch.int32)
    junk = 0 if mode == "zero" else 10 ** 9      # behind a row's frames: tokens that would be out of range / NaN embeddings
    tok = torch.full((len(rows), Tfm, n_q), junk, dtype=torch.int64)
    embs = torch.full((len(rows), Tfm, D), float("nan") if mode != "zero" else 0.0)
    for b, (_, ref, _) in enumerate(rows):
        tok[b, :fl[b]] = torch.from_numpy(ref["indices"][:, 0]).t()
        embs[b, :fl[b]] = torch.from_numpy(np.asarray(ref["quantized"][0]))
    w2, emb = e.decode_codes(tok, lengths=fl)
    w3 = e.decode_emb(embs, lengths=fl)
    e.check_status(sync=True)
    for v in (w2, emb, w3):
        assert bool(torch.isfinite(v).all())
    return got, dict(w2=w2, emb=emb, w3=w3), lens


GOLDEN_BATCHES = {
    # recipe: (rows from committed one-utterance fixtures (name, row), seeded extra rows (len, seed) checked against the oracle)
    "ds320": ([("ds320_wav_libritts_5105", 0), ("ds320_b1_t16000", 0), ("ds320_wav_libritts_8230", 0)], [(700, 5)]),
    # the 10 s recording: 40 statistics segments per row at the first layers, 79 column segments of the staging kernel
    "ds640": ([("ds640_b2_t16000", 1), ("ds640_wav_libritts_8230", 0), ("ds640_b2_t16000", 0), ("ds640_wav_libritts_5105", 0),
               ("ds640_wav_jamendo_0027", 0)], []),
    "ds640bw": ([("ds640_b1_t9999_bw4000", 0)], [(16000, 6), (4321, 7)]),
    "ds320wn": ([("ds320wn_b1_t12000", 0)], [(4321, 8), (700, 9), (16000, 10)]),
    "ss320": ([("ss320_b1_t8000", 0)], [(9999, 11), (333, 12)]),
    "ss320nc": ([("ss320nc_b1_t8000", 0)], [(9999, 13), (333, 14)]),
    "tinyst": ([("tinyst_b3_t1003", 2), ("tinyst_b3_t1003", 0), ("tinyst_b3_t1003", 1)], [(257, 15), (2000, 16)]),
    "ds320cd64": ([("ds320cd64_b1_t8000", 0)], [(5000, 17), (12000, 18)]),
}
# (MANIFEST.json lists no fuzz* case for the ds320 recipe: every fuzz case has a configuration of its own)
assert not [n for n, c in MAN["cases"].items() if n.startswith("fuzz") and c.get("config") == "ds320"]


@pytest.mark.parametrize("mode", ["zero", "nan", "wrap"])
@pytest.mark.parametrize("key", sorted(GOLDEN_BATCHES))
def test_ragged_batch_rows_equal_the_one_utterance_goldens(key, mode):
    fixtures, extra = GOLDEN_BATCHES[key]
    c0 = MAN["cases"][fixtures[0][0]]
    cfg_name, seed, decay, n_q, ch = c0["config"], c0["weight_seed"], c0["codebook_decay"], c0["n_q"], c0.get("channels", 1)
    bw = c0.get("bit_width")
    m = engine_for(cfg_name, seed, decay)
    cfg, arch, sd = state_for(cfg_name, seed, decay)
    rows = []
    for name, row in fixtures:
        c = MAN["cases"][name]
        assert (c["config"], c["weight_seed"], c["codebook_decay"], c["n_q"]) == (cfg_name, seed, decay, n_q)
        rows.append(_ref_from_golden(name, row))
    for n, s in extra:
        rows.append(_seeded_row(cfg_name, seed, decay, n, s, ch, bw))
    rows = rows[1::2] + rows[0::2]               # mixed order: neither sorted by length nor fixtures first
    got, dec, lens = _run(m, rows, n_q, mode)
    for b, (_, ref, tag) in enumerate(rows):
        _check_row(m, sd, arch, f"{tag}[{mode}]", b, lens[b], got, dec, ref)


@pytest.mark.parametrize("cfg_name,seed", [("tiny", 7), ("tinywn", 9), ("tinyss", 5)])
def test_ragged_edge_lengths_against_the_oracle(cfg_name, seed):
    m = engine_for(cfg_name, seed)
    cfg, arch, sd = state_for(cfg_name, seed)
    hop = m.engine.hop_length
    lens = [1, 2, 5, 6, hop - 1, hop, hop + 1, 3 * hop + 7, 5 * hop, 7 * hop - 1, 9 * hop + 1, 12 * hop + 3, 16 * hop, 21 * hop + 5,
            27 * hop - 2, 33 * hop + 1, 40 * hop]
    assert len(lens) == 17
    ch = 2 if arch.input_channels == 2 and arch.model_type == "encodec" else 1
    rows = [_ref_from_oracle(cfg_name, seed, 1.0, audio(1, n, 900 + i, "noise" if i % 2 else "tones", ch)[0], None, f"{cfg_name}:len{n}")
            for i, n in enumerate(lens)]
    rows = rows[3:] + rows[:3]
    got, dec, lens2 = _run(m, rows, arch.num_quantizers, "nan")
    for b, (_, ref, tag) in enumerate(rows):
        _check_row(m, sd, arch, tag, b, lens2[b], got, dec, ref)


@pytest.mark.parametrize("cfg_name,seed,n", [("ds320", 0, 9999), ("ds320wn", 0, 4321), ("ss320", 0, 700), ("tiny", 7, 333)])
def test_ragged_rows_do_not_depend_on_the_batch_around_them(cfg_name, seed, n):
    """One utterance alone (Tmax = len), as row 0 of B = 2 with a longer companion, as row 5 of B = 8 among shorter and longer ones, as
    row 11 of B = 16 next to a 10 s row (Tmax 160000): every valid output bit-identical.  No tolerance."""
    m = engine_for(cfg_name, seed)
    e, n_q = m.engine, m.arch.num_quantizers
    x = audio(1, n, 77, "tones")[0]
    others = [audio(1, k, 200 + k, "noise")[0] for k in (2 * n + 13, n // 3 + 1, n + 1, 5, n - 1, 3 * n, n // 2 + 7)]
    long16 = [audio(1, k, 300 + i, "noise")[0] for i, k in enumerate((16000, 160000, 77, 48001, n, 31999, 1, 9600, 123456, 640, 80000, 5000, 2 * n,
                                                                      40000, 321))]
    batches = [([x], 0), ([x, others[0]], 0), (others[1:6] + [x] + others[5:7], 5), (long16[:11] + [x] + long16[11:], 11)]
    outs = []
    for rows, b in batches:
        lens = [r.shape[-1] for r in rows]
        wav = _fill(rows, max(lens), "nan" if len(rows) > 1 else "zero")
        L = torch.tensor(lens, dtype=torch.int32)
        r = e.encode_decode(wav, n_q, use_scale=True, lengths=L)
        r1 = e.encode(wav, n_q, want_enc_out=True, lengths=L)
        Tf = e.frames(n)
        fl = torch.tensor([e.frames(k) for k in lens], dtype=torch.int32)
        w2, emb = e.decode_codes(r["codes"].permute(1, 2, 0).contiguous(), lengths=fl)
        w3 = e.decode_emb(r["quantized"], lengths=fl)
        e.check_status(sync=True)
        outs.append(dict(codes=r["codes"][:, b, :Tf], quantized=r["quantized"][b, :Tf], sub_quants=r["sub_quants"][:, b, :, :Tf],
                         scale=r["scale"][b] if r["scale"] is not None else torch.zeros(1), recon=r["recon"][b, :, :n],
                         enc_out=r1["enc_out"][b, :Tf], codes1=r1["codes"][:, b, :Tf], w2=w2[b, :, :Tf * e.hop_length], emb=emb[b, :Tf],
                         w3=w3[b, :, :Tf * e.hop_length]))
    for k, v in outs[0].items():
        assert bool(torch.isfinite(v.float()).all()), k
        for i in (1, 2, 3):
            assert torch.equal(v, outs[i][k]), (k, i, float((v.float() - outs[i][k].float()).abs().max()))


def test_ragged_length_errors_are_reported_and_the_engine_stays_usable():
    from funcodec_amd.engine import EngineError
    m = engine_for("tiny", 7)
    e = m.engine
    wav = audio(2, 500, 3, "noise")
    good = e.encode(wav, 2, lengths=torch.tensor([500, 123], dtype=torch.int32))
    e.check_status(sync=True)
    for bad in (0, 501):
        e.encode(wav, 2, lengths=torch.tensor([500, bad], dtype=torch.int32))
        with pytest.raises(EngineError, match="length"):
            e.check_status(sync=True)
        e.check_status(sync=True)                 # reported once, then cleared
    again = e.encode(wav, 2, lengths=torch.tensor([500, 123], dtype=torch.int32))
    e.check_status(sync=True)
    assert torch.equal(again["codes"], good["codes"])
    with pytest.raises(EngineError, match="one entry per row"):
        e.encode(wav, 2, lengths=torch.tensor([500], dtype=torch.int32))


@pytest.mark.parametrize("cfg_name,key", [("ds320tf", "seq_model: transformer"), ("ds320q0", "q0_ds_ratio"), ("ds320seg", "segment_dur"),
                                          ("freqmp", "freq_codec")])
def test_ragged_refused_architectures_name_the_key(cfg_name, key):
    from funcodec_amd.engine import EngineError
    from helpers import freq_engine_for
    m = freq_engine_for(cfg_name, 0) if cfg_name == "freqmp" else engine_for(cfg_name, 0)
    wav = audio(2, 4000, 3, "noise")
    with pytest.raises(EngineError, match=key):
        m.inference(wav.cuda(), speech_lengths=torch.tensor([4000, 1000]))
    if cfg_name != "ds320seg":                    # segments are a host loop: the library itself has no such notion
        e = m.engine
        assert e.lib.fc_ragged_workspace_bytes(e._h, 2, 4000) == 0
        # the library refuses on its own, whatever the host checked: the four calls, before they look at an argument
        x = wav.cuda()
        L = torch.tensor([4000, 1000], dtype=torch.int32, device="cuda")
        codes = torch.zeros(1, 2, e.frames(4000), dtype=torch.int64, device="cuda")
        ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        P = lambda t: t.data_ptr()      # noqa: E731
        calls = [e.lib.fc_encode_ragged(e._h, P(x), P(L), 2, 4000, 1, P(codes), None, None, None, None, P(ws), ws.numel(), None),
                 e.lib.fc_encode_decode_ragged(e._h, P(x), P(L), 2, 4000, 1, 1, P(codes), None, None, None, P(x), P(ws), ws.numel(), None),
                 e.lib.fc_decode_codes_ragged(e._h, P(codes), P(L), 2, 1, 1, 1, P(x), None, P(ws), ws.numel(), None),
                 e.lib.fc_decode_emb_ragged(e._h, P(x), None, P(L), 2, 1, 1, P(x), P(ws), ws.numel(), None)]
        for rc in calls:
            assert rc != 0
        e.lib.fc_encode_ragged(e._h, P(x), P(L), 2, 4000, 1, P(codes), None, None, None, None, P(ws), ws.numel(), None)
        assert key in e.lib.fc_last_error().decode()
    m.inference(wav.cuda())                       # the offline call is untouched
    m.engine.check_status(sync=True)


def test_ragged_host_keywords_reach_the_engine():
    """EncodecMI355X.inference* with speech_lengths / token_lengths, and Speech2Token-style pass-through of the same rows."""
    m = engine_for("tinywn", 9)
    n = [777, 300]
    rows = [audio(1, k, 30 + k, "tones")[0] for k in n]
    wav = _fill(rows, 777, "nan").cuda()
    ret = m.inference(wav, speech_lengths=torch.tensor(n))
    enc = m.inference_encoding(wav, speech_lengths=torch.tensor(n))
    assert torch.equal(enc["code_indices"][0], ret["code_indices"][0])
    alone = m.inference(rows[1][None].cuda())
    Tf = m.engine.frames(300)
    assert torch.equal(ret["code_indices"][0][:, 1, :Tf], alone["code_indices"][0][:, 0])
    assert rms(ret["recon_speech"][1, :, :300], alone["recon_speech"][0]) < WAV_RMS_TOL
    fl = torch.tensor([m.engine.frames(k) for k in n])
    d = m.inference_decoding(ret["code_indices"][0].permute(1, 2, 0).contiguous(), token_lengths=fl)
    d2 = m.inference_decoding_emb(ret["code_embeddings"][0][0], token_lengths=fl)
    assert torch.equal(d["recon_speech"], d2["recon_speech"])
    assert float(d["recon_speech"][1, :, Tf * m.engine.hop_length:].abs().sum()) == 0.0
    m.engine.check_status(sync=True)


def _write_scp(tmp_path, lens, seed):
    from funcodec_amd import io as fio
    wavs = audio(len(lens), max(lens), seed, "tones")
    scp = tmp_path / "wav.scp"
    with open(scp, "wt") as f:
        for i, n in enumerate(lens):
            p = str(tmp_path / f"u{i}.wav")
            fio.save_audio(wavs[i:i + 1, :n], p, 16000, rescale=False)
            f.write(f"u{i} {p}\n")
    return scp


def _same_files(a, b, keys, wav=True):
    import os
    from funcodec_amd import io as fio
    assert open(os.path.join(a, "codecs.txt")).read() == open(os.path.join(b, "codecs.txt")).read()
    for k in keys if wav else []:
        ya, sa = fio.read_wav(os.path.join(a, k + ".wav"))
        yb, sb = fio.read_wav(os.path.join(b, k + ".wav"))
        assert sa == sb and ya.shape == yb.shape and np.array_equal(ya, yb), k


@pytest.mark.parametrize("cfg_name", ["ds320", "ds320wn"])
def test_cli_length_aware_batches_write_what_batch_size_one_writes(tmp_path, cfg_name):
    """Four wav files of different lengths through the CLI: with length_aware, batch_size 4 writes the codecs.txt and the wav files
    (sample for sample) that batch_size 1 writes, for run_mod inference, encode and decode, from the command line and through
    param_dict; with the flag off, batch_size 4 writes what the wrap-padded batch gives, as before (the expectation of
    test_gpu_parity.py::test_cli_encoding_decoding_pipeline)."""
    import os
    from funcodec_amd import io as fio
    from funcodec_amd.bin.codec_inference import inference_modelscope, main
    from funcodec_amd.synth import make_checkpoint
    cfg_path, pth_path = make_checkpoint(str(tmp_path / "model"), cfg_name, 0)
    lens = [4000, 6400, 3333, 901]
    keys = [f"u{i}" for i in range(4)]
    scp = _write_scp(tmp_path, lens, 78)
    data = f"{scp},speech,sound"

    def cli(out, bs, run_mod, data, extra=()):
        main(["--ngpu", "1", "--gpuid_list", "0", "--output_dir", out, "--batch_size", str(bs), "--sampling_rate", "16000",
              "--config_file", cfg_path, "--model_file", pth_path, "--bit_width", "8000", "--need_indices", "true",
              "--run_mod", run_mod, "--data_path_and_name_and_type", data] + list(extra))
        return out

    aware = ("--length_aware", "true")
    # inference (codes + reconstruction), from the command line
    a4 = cli(str(tmp_path / "inf4.1"), 4, "inference", data, aware)
    a1 = cli(str(tmp_path / "inf1.1"), 1, "inference", data, aware)
    _same_files(a4, a1, keys)
    got = {k: fio.load_codec_json(v) for k, v in fio.read_scp(os.path.join(a4, "codecs.txt"))}
    for k, n in zip(keys, lens):
        y, sr = fio.read_wav(os.path.join(a4, k + ".wav"))
        assert sr == 16000 and y.shape[0] == n and got[k].shape == (-(-n // 320), 16)
    # ... and it is each utterance ALONE: the oracle on one utterance at a time
    orc = oracle_for(cfg_name, 0)
    for k, n in zip(keys, lens):
        x, _ = fio.read_wav(str(tmp_path / f"{k}.wav"))
        o = orc.inference(torch.from_numpy(x)[None], bit_width=8000, use_scale=True)
        assert np.array_equal(got[k], o["code_indices"][0][:, 0].numpy().T), k
    # the same through param_dict of the pipeline (batch 4 and batch 3: another grouping of the same files)
    for bs in (4, 3):
        out = str(tmp_path / f"pd{bs}.1")
        pipe = inference_modelscope(output_dir=out, batch_size=bs, ngpu=1, sampling_rate=16000, config_file=cfg_path, model_file=pth_path,
                                    bit_width=8000, need_indices=True, run_mod="inference")
        pipe([(str(scp), "speech", "sound")], param_dict={"length_aware": True})
        _same_files(out, a1, keys)
    # encode: codes only
    e4 = cli(str(tmp_path / "enc4.1"), 4, "encode", data, aware)
    e1 = cli(str(tmp_path / "enc1.1"), 1, "encode", data, aware)
    _same_files(e4, e1, keys, wav=False)
    assert open(os.path.join(e4, "codecs.txt")).read() == open(os.path.join(a1, "codecs.txt")).read()
    # decode from codecs.txt: the lengths are frames there
    cdata = f"{os.path.join(a1, 'codecs.txt')},speech,codec_json"
    d4 = cli(str(tmp_path / "dec4.1"), 4, "decode", cdata, aware)
    d1 = cli(str(tmp_path / "dec1.1"), 1, "decode", cdata, aware)
    _same_files(d4, d1, keys)
    # flag off: batch_size 4 is the offline call on the wrap-padded batch, as on the parent commit
    off = cli(str(tmp_path / "off4.1"), 4, "inference", data, ("--use_scale", "false"))
    (bkeys, b), = list(fio.iter_batches([(str(scp), "speech", "sound")], 4))
    o = orc.inference(b["speech"], bit_width=8000, use_scale=False)
    goff = {k: fio.load_codec_json(v) for k, v in fio.read_scp(os.path.join(off, "codecs.txt"))}
    for i, k in enumerate(bkeys):
        n = int(b["speech_lengths"][i])
        cl = -(-n // 320)
        assert np.array_equal(goff[k], o["code_indices"][0][:, i, :cl].numpy().T), k
        y, _ = fio.read_wav(os.path.join(off, k + ".wav"))
        r = o["recon_speech"][i, 0, :n].numpy()
        r = r * min(0.99 / np.abs(r).max(), 1.0)
        assert y.shape[0] == n and np.abs(y - r).max() < 2.0 / 32768, k
    # lengths count file samples: with resampling the switch refuses instead of guessing
    with pytest.raises(NotImplementedError, match="length_aware"):
        cli(str(tmp_path / "rs.1"), 4, "inference", data, aware + ("--file_sampling_rate", "8000"))
