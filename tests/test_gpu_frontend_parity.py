"""The chain every audio-understanding request enters through, on the device, against the float64 references of
tests/frontend_refs.py under the project's bar kr.bar(E, scale) = max(4 E, 8 * 2^-24 * scale): `reason_tokenizer.resample`
(the product's function: one exact-fp32 ua2_linear launch per chunk of rows), ua2_logmel on all 80 x 3000 values of every clip, and
the WhisperEncoder mirror in both plans.  E is the error of the SAME formula replayed in fp32 on the host (resample_ref / logmel_ref
/ encoder_ref in float32) on the very input of the case, scale = max(1, max |ref|); for the bf16 encoder E is the error of the
float64 replay whose GEMM operands and cached k, v are rounded to bf16 (whisper_ref.encoder_ref(rnd=kr.bf16_once)).  Every case
prints `PARITY <family> <case>: err .. E .. bar .. err/bar ..`; a captured run is profiles/frontend_parity.txt.
tests/test_frontend_refs_host.py pins the references on the CPU and shows that the wrong models exceed these bars on these inputs.

Worst err / bar per family on an MI355X (profiles/frontend_parity.txt):
  resample                 0.42  (16 -> 24 kHz, the amplitude-3e4 clip; noise at 0.3: 0.35; every impulse exact)
  logmel, max | rms        0.59 | 0.26  (both on clip a; every edge length <= 0.38 | 0.21; clips c and `floor` exact)
  encoder fp32             0.21  (P = 1500, last hidden state; stems <= 0.15)
  encoder bf16             0.28  (P = 1500, last hidden state): err / E_model 0.93 .. 1.13 on the last hidden state and 1.000 on
                           every stem — the model needed no correction
No case failed on the device: no kernel was changed.

Long files.  `tokenize` resamples a whole file in one call, so the GEMM's M grows with the file (one row per orig / gcd input
samples).  Read from the launch code (csrc/ua2_gemm.hip): the prep kernels and the tiled form (launch_gemm) put their row blocks on
grid x, which HIP bounds at 2^31 - 1; the decode kernel serves a launch only up to ua2_gemv_rows_preferred rows (gemm_takes); but
launch_skinny puts ceil(ceil(M / 16) / 4) workgroups on grid y, 65 535 at most, i.e. M <= 4 194 240 rows, and nothing in it or in
launch_dt bounds M.  Whether a launch takes that form is choose_skinny's cost model (t_skinny <= t_tiled): with today's constants
it loses at the product's rate pairs for every M (N K <= 26 240: 8 + 4 ceil(M / 64) us against max(5 + 0.55 K / 16, 2 M N K / 45e6) us), but it wins
for every large M once N K >= 1.96e6 (a file whose rate shares only a small factor with 24 000), and UA2_SKINNY_MAX_ROWS hands it any
M outright — a cost table is not a guarantee, and a refused launch would fail the whole file.  So `resample` bounds M itself: the
rows go through in chunks of `max_rows` (2^20 by default: 16 384 on grid y), which is data movement only because a row's bits do not
depend on the rows beside it — test_resample_chunked_is_bitwise_unchunked and test_resample_prefix_property hold that.  No test here
launches a configuration the code shows would be refused."""
import functools
import math

import pytest
import torch

import frontend_refs as fr
import kernel_refs as kr
import whisper_ref as wr

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
SENT = 12352.0                                  # finite, and no log-mel value or workgroup maximum reaches it
GUARD = 64                                      # floats on either side of a guarded buffer (keeps 16-byte alignment)
STALE = 3.0e4                                   # what surrounds the input clip: a read outside it cannot go unnoticed


def _line(family, case, err, e, bar, what="E_ref"):
    print(f"PARITY {family} {case}: err {err:.3e} {what} {e:.3e} bar {bar:.3e} err/bar {err / bar:.3f}")


def _rt():
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film import reason_tokenizer
    return reason_tokenizer


# ---- resampler --------------------------------------------------------------------------------------------------------------

def _case(name):
    orig, new, L = fr.resample_cases()[name]
    return orig, new, (L if L is not None else fr.segment_len())


def _resample(x, orig, new, **kw):
    """The product's resample on a host tensor [C, L] -> host result; the input must come back unchanged."""
    xd = x.cuda()
    keep = xd.clone()
    y = _rt().resample(xd, orig, new, **kw)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep), "resample changed its input"
    return y.cpu()


@pytest.mark.parametrize("name", list(fr.resample_cases()))
def test_resample_against_float64(name):
    orig, new, L = _case(name)
    inputs = fr.resample_inputs(L, 7900 + list(fr.resample_cases()).index(name))
    alone, failed = {}, []
    for kind, x in inputs.items():
        got = _resample(x, orig, new)
        assert got.dtype == F32 and got.shape == (1, math.ceil(new * L / orig)), (got.shape, L)
        ref = fr.resample_ref(x, orig, new, F64)
        e = float((fr.resample_ref(x, orig, new, F32).to(F64) - ref).abs().max())
        bar = kr.bar(e, max(1.0, float(ref.abs().max())))
        err = kr.abs_err(got, ref)
        _line("resample", f"{name} {kind}", err, e, bar)
        if not err <= bar:
            failed.append((kind, err, bar))
        alone[kind] = got
    assert not failed, failed
    # three rows at once: every row has the bits of the same row run alone
    kinds = ["noise", "loud", "impulse_last"]
    got3 = _resample(torch.cat([inputs[k] for k in kinds]), orig, new)
    assert got3.shape == (3, math.ceil(new * L / orig))
    for i, k in enumerate(kinds):
        assert torch.equal(got3[i], alone[k][0]), f"row {i} ({k}) of three differs from the row run alone"


def test_resample_equal_rates_return_the_argument():
    x = torch.zeros(1, 100, device="cuda")
    assert _rt().resample(x, 24000, 24000) is x and _rt().resample(x, 16000, 16000.0) is x


@pytest.mark.parametrize("orig,new,L,L1", [(24000, 16000, 26000, 10001), (24000, 16000, 26000, 49), (22050, 24000, 9000, 4099), (48000, 24000, 9001, 2050)])
def test_resample_prefix_property(orig, new, L, L1):
    """Rows of the GEMM do not see each other: resample(x[:, :L1]) is resample(x), bit for bit, on every output whose taps lie inside
    the first L1 samples — across the two launches' different M (and whatever form of ua2_linear each M selects)."""
    x = fr.resample_inputs(L, 7950)["noise"]
    full, head = _resample(x, orig, new), _resample(x[:, :L1].contiguous(), orig, new)
    k = fr.prefix_outputs(L1, orig, new)
    assert 0 < k <= head.shape[1] == math.ceil(new * L1 / orig)
    assert torch.equal(full[:, :k], head[:, :k])


@pytest.mark.parametrize("chunk", [5, 16, 1000, 4096])
def test_resample_chunked_is_bitwise_unchunked(chunk):
    """L = 26 000 at 24 -> 16 kHz is 8667 rows: chunks of 5 and 16 rows go to the decode kernel, 1000 and 4096 to the tiled one with a
    ragged last chunk; the unchunked launch is the product's default (max_rows above the row count)."""
    x = fr.resample_inputs(26000, 7960)["noise"]
    whole = _resample(x, 24000, 16000)
    assert torch.equal(_resample(x, 24000, 16000, max_rows=chunk), whole)
    assert torch.equal(_resample(x, 24000, 16000, max_rows=8667), whole) and _rt().RESAMPLE_MAX_ROWS > 8667
    assert _rt().RESAMPLE_MAX_ROWS <= 65535 * 64                      # launch_skinny's grid y, whatever the cost model picks
    with pytest.raises(ValueError):
        _rt().resample(x.cuda(), 24000, 16000, max_rows=0)


# ---- ua2_logmel -------------------------------------------------------------------------------------------------------------

def _guarded(n, fill=SENT):
    buf = torch.full((n + 2 * GUARD,), fill, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _guards_keep(buf, fill=SENT):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


@functools.lru_cache(maxsize=None)
def _tables():
    from uniaudio2_amd import ops
    basis, fb = ops.logmel_tables_host()
    return basis.float().contiguous().cuda(), fb.float().contiguous().cuda()


def _launch_logmel(x, B=None, n_samples=None, ws_short=0):
    """lib.ua2_logmel on a host batch x [B, N] with buffers the test owns.  -> (return code, out [B, 80, 3000] host, out buffer, ws
    buffer, ws view).  The clip sits between two bands of 3e4; out and ws between two bands of the sentinel they are filled with."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import lib
    Bx, N = x.shape
    B = Bx if B is None else B
    n_samples = N if n_samples is None else n_samples
    basis, fb = _tables()
    xbuf, xd = _guarded(Bx * N, STALE)
    xd.copy_(x.reshape(-1))
    keep = xbuf.clone()
    obuf, out = _guarded(Bx * wr.N_MELS * wr.N_FRAMES)
    ws_bytes = lib.ua2_logmel_workspace_bytes(Bx)
    assert ws_bytes == Bx * 188 * 4
    wbuf, ws = _guarded(ws_bytes // 4)
    rc = lib.ua2_logmel(out.data_ptr(), xd.data_ptr(), B, n_samples, basis.data_ptr(), fb.data_ptr(), ws.data_ptr(), ws_bytes - ws_short,
                        ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(xbuf, keep), "ua2_logmel changed its input"
    assert _guards_keep(obuf) and _guards_keep(wbuf), "ua2_logmel wrote outside out / ws"
    return rc, out.view(Bx, wr.N_MELS, wr.N_FRAMES).cpu(), obuf, wbuf, ws


def _logmel(x):
    rc, got, _, _, ws = _launch_logmel(x)
    assert rc == 0
    assert not bool((got == SENT).any()), "a value of out was never written"
    assert not bool((ws == SENT).any()) and bool(torch.isfinite(ws).all()), "a workgroup maximum was never written"
    return got


def _hold_logmel(case, got, ref, emax, erms, scale):
    err, rms = fr.max_rms(got, ref)
    bar, rbar = kr.bar(emax, scale), kr.bar(erms, scale)
    _line("logmel", f"{case} max", err, emax, bar)
    _line("logmel", f"{case} rms", rms, erms, rbar)
    assert emax <= fr.LOGMEL_MAX_E_REF
    assert err <= bar and rms <= rbar, (case, err, bar, rms, rbar)


@functools.lru_cache(maxsize=None)
def _logmel_single(case):
    return _logmel(torch.from_numpy(fr.logmel_clip(case))[None])[0]


@pytest.mark.parametrize("case", fr.LOGMEL_CASES)
def test_logmel_all_values_against_float64(case):
    got = _logmel_single(case)
    ref, emax, erms, scale = fr.logmel_refs(case)
    _hold_logmel(case, got, ref, emax, erms, scale)
    if case in ("c", "floor"):
        assert torch.equal(got, torch.full_like(got, -1.5))
    else:
        assert float(got.min()) >= float(got.max()) - 2.0 - 1e-6           # the max - 8 clamp, after (x + 4) / 4


def test_logmel_batch_rows_are_the_single_clips():
    """B = 3 at 480 160 samples, different content per row: the clip stride past the truncation point, and every clip's own maximum."""
    x = fr.logmel_batch()
    got = _logmel(x)
    ref, emax, erms, scale = fr.logmel_stats(x)
    for i in range(3):
        assert torch.equal(got[i], _logmel(x[i:i + 1].contiguous())[0]), f"row {i} of the batch differs from its single-clip launch"
        _hold_logmel(f"batch row {i}", got[i], ref[i], emax[i], erms[i], scale[i])
        assert abs(float(got[i].max()) - float(ref[i].max())) <= kr.bar(emax[i], scale[i])
        assert float(got[i].min()) >= float(got[i].max()) - 2.0 - 1e-6                                   # each clip clamps at ITS maximum - 8 ...
        assert abs(float(got[i].min()) - float(ref[i].min())) <= kr.bar(emax[i], scale[i])              # ... where the reference does


@pytest.mark.parametrize("what", ["B=0", "n_samples=0", "workspace one byte short"])
def test_logmel_refusals_launch_nothing(what):
    from uniaudio2_amd._lib import lib
    x = torch.from_numpy(fr.logmel_clip("n2361"))[None]
    kw = {"B=0": dict(B=0), "n_samples=0": dict(n_samples=0), "workspace one byte short": dict(ws_short=1)}[what]
    rc, got, obuf, wbuf, _ = _launch_logmel(x, **kw)
    assert rc != 0 and b"ua2_logmel" in lib.ua2_last_error()
    assert bool((obuf == SENT).all()) and bool((wbuf == SENT).all()), "a refused call wrote something"


# ---- WhisperEncoder mirror --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _encoder(name, dtype):
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.modeling_whisper import WhisperEncoder
    cfg, sd, mels = fr.encoder_inputs(name)
    enc = WhisperEncoder(cfg)
    enc.load_state_dict(sd, strict=True)
    return enc.cuda().prepare(dtype), mels.cuda()


def _run_encoder(name, dtype):
    enc, mels = _encoder(name, dtype)
    g = fr.ENCODER_GEOMS[name]
    B, P, d = g["B"], g["cfg"]["max_source_positions"], g["cfg"]["d_model"]
    assert mels.shape == (B, 80, g["T"]) and (g["T"] - 1) // 2 + 1 == P
    last = enc(mels)
    stem, P_ = enc.stem(mels)
    assert P_ == P and last.shape == (B, P, d) and last.dtype == F32
    alone = enc(mels[:1].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(alone[0], last[0]), "row 0 of the batch differs from the row run alone"
    return last.cpu(), stem.view(B, P, d).cpu()


@pytest.mark.parametrize("name", list(fr.ENCODER_GEOMS))
def test_encoder_fp32_against_float64(name):
    last, stem = _run_encoder(name, F32)
    r = fr.encoder_refs(name)
    failed = []
    for what, got in (("stem", stem), ("last", last)):
        ref, e = r[what], r["e32_" + what]
        bar = kr.bar(e, max(1.0, float(ref.abs().max())))
        err = kr.abs_err(got, ref)
        _line("encoder fp32", f"{name} {what}", err, e, bar)
        if not err <= bar:
            failed.append((what, err, bar))
    assert not failed, failed


@pytest.mark.parametrize("name", list(fr.ENCODER_GEOMS))
def test_encoder_bf16_against_the_rounding_model(name):
    """The bf16 plan against float64 under the bar of its model: both operands of every GEMM and the cached k, v rounded to bf16
    once, everything else wide (whisper_ref.encoder_ref(rnd=kr.bf16_once) in float64).  The printed err / E_model is the record."""
    last, stem = _run_encoder(name, BF16)
    r = fr.encoder_refs(name)
    failed = []
    for what, got in (("stem", stem), ("last", last)):
        ref, e = r[what], r["em_" + what]
        bar = kr.bar(e, max(1.0, float(ref.abs().max())))
        err = kr.abs_err(got, ref)
        _line("encoder bf16", f"{name} {what}", err, e, bar, what="E_model")
        print(f"        err / E_model {err / e:.3f}")
        if not err <= bar:
            failed.append((what, err, bar))
    assert not failed, failed


@pytest.mark.parametrize("name", ["oddT", "p72"])
def test_packed_handover_is_bitwise_the_row_major_route(name):
    """modeling_whisper.WhisperEncoderLayer.run: at M > 16 the bf16 plan lets attention and fc1's GELU write their consumer's operand
    in fragment order ("identical bits, two launches less").  The four launches of the row-major branch, issued by hand on the same
    q and the same K / V pools with the same kv.groups, must give the packed branch's bits."""
    from uniaudio2_amd._lib import EPI_GELU, EPI_QKV_ROPE, EPI_RESIDUAL, ROPE_NONE
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models._dense import DenseKV
    enc, mels = _encoder(name, BF16)
    h0, P = enc.stem(mels)
    B, d = mels.shape[0], enc.d_model
    M = B * P
    kv = DenseKV(B, P, enc.heads, d // enc.heads, BF16, h0.device)
    layer = enc.layers[0]
    p = layer._p
    assert kv.groups is not None and M > 16 and d % 32 == 0 and p["fc2"].K % 32 == 0, "this geometry does not take the packed branch"
    packed = layer.run(h0.clone(), kv).clone()
    h = h0.clone()
    q = torch.empty(M, d, dtype=F32, device=h.device)
    p["qkv"](h, epilogue=EPI_QKV_ROPE, norm=p["ln1"], rope_mode=ROPE_NONE, row_pos=kv.row_pos, row_seq=kv.row_seq, q_out=q, kv=kv.geom)
    o = kv.attend(q)
    p["out"](o, epilogue=EPI_RESIDUAL, resid=h, y=h)
    f = p["fc1"](h, epilogue=EPI_GELU, norm=p["ln2"])
    p["fc2"](f, epilogue=EPI_RESIDUAL, resid=h, y=h)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(packed).all()) and not torch.equal(packed, h0)
    assert torch.equal(packed, h), f"packed hand-over differs from the row-major route: max |diff| {float((packed - h).abs().max()):.3e}"
