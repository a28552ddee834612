"""GPT-2-117M end to end (BASELINE config 4): synthetic seeded f16 weights.

Checkers (test infrastructure, oracle/Makefile `gpt2`):
  * oracle/_ref/gpt-2-backend -- the reference's own examples/gpt-2/main-backend.cpp, unmodified,
    on the reference CPU backend;
  * oracle/_ref/libgpt2_ref.so / gpt-2-mi355x-ref -- this repo's GPT-2 driver linked against the
    reference libggml, so the reference CPU ops compute the logits.

CPU tests pin the driver to the reference program (identical generated text for a seed, i.e. same
graph, tokenizer and sampler); GPU tests compare teacher-forced MI355X logits with the reference
CPU logits. BASELINE's bar is max |d| / max |ref| <= 1e-3 (met by the default fast decode GEMVs of
the f16 model; a quantized model's graphs run in the reference order by default, bit-identical);
with mmv_order=1 (decode GEMVs in the reference's summation order) the decode-path logits (prompt
batches of <= 8 tokens, then single tokens) are bit-identical to the CPU's, and the product CLI on
MI355X samples exactly the text the reference program samples on the CPU.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

from ggml_mi355x import ggml as G
from ggml_mi355x import gpt2

REF = os.path.join(REPO, "oracle", "_ref")
REF_BIN = os.path.join(REF, "gpt-2-backend")
OUR_REF_BIN = os.path.join(REF, "gpt-2-mi355x-ref")
REF_GGML = os.path.join(REF, "libggml_ref.so")
REF_GPT2 = os.path.join(REF, "libgpt2_ref.so")
OUR_BIN = os.path.join(REPO, "ggml-imax_amd", "bin", "gpt-2-mi355x")

PROMPT = "Once upon a time the cat sat on the mat and the dog"
LOGIT_TOL = 1e-3


@pytest.fixture(scope="module")
def model_path():
    return gpt2.ensure_model()


def _text(out: str) -> str:
    # the generated text sits between the "first 8 tokens" line and the timing block
    body = out.split("first 8 tokens:", 1)[1].split("\n", 1)[1]
    return body.split("main:     load time", 1)[0].strip()


def test_synthetic_model_format(model_path):
    size = os.path.getsize(model_path)
    assert size > 239 * 1024 * 1024
    with open(model_path, "rb") as f:
        hdr = np.frombuffer(f.read(32), dtype=np.int32)
    assert hdr[0] == 0x67676D6C
    assert list(hdr[1:7]) == [50257, 1024, 768, 12, 12, 1]


@pytest.mark.skipif(not (os.path.exists(REF_BIN) and os.path.exists(OUR_REF_BIN)), reason="make -C oracle gpt2")
def test_driver_matches_reference_program(model_path):
    """Same seed + prompt: the reference program and our driver (both on reference CPU ops) print
    the same tokens -- our graph, tokenizer and sampler mirror examples/gpt-2 exactly."""
    args = ["-m", model_path, "-p", PROMPT, "-n", "24", "-s", "7", "-t", "4"]
    ref = subprocess.run([REF_BIN] + args, capture_output=True, text=True, timeout=300)
    ours = subprocess.run([OUR_REF_BIN] + args, capture_output=True, text=True, timeout=300)
    assert ref.returncode == 0, ref.stderr[-2000:]
    assert ours.returncode == 0, ours.stderr[-2000:]
    assert "model size  =   239.08 MB" in ref.stdout
    assert "model size  =   239.08 MB" in ours.stdout
    t_ref, t_ours = _text(ref.stdout), _text(ours.stdout)
    assert len(t_ref) > len(PROMPT)
    assert t_ref == t_ours


def _ref_model(path):
    return _ref_model_nb(path, 8)


def _ref_model_nb(path, n_batch):
    ref = G.Lib([REF_GGML, REF_GPT2], isolated=True)
    be = ref.ggml_backend_cpu_init()
    ref.ggml_backend_cpu_set_n_threads(be, min(16, os.cpu_count() or 1))
    return ref, be, gpt2.Model(ref, path, be, n_ctx=1024, n_batch=n_batch)


@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
def test_reference_driver_tokenizer_roundtrip(model_path):
    ref, be, m = _ref_model(model_path)
    try:
        toks = m.tokenize(PROMPT)
        assert len(toks) > 4
        assert b"".join(m.token_text(t) for t in toks).decode() == PROMPT
        logits = m.eval(0, toks[:8])
        assert logits.shape == (1, 50257) and np.isfinite(logits).all()
    finally:
        m.free()
        ref.ggml_backend_free(be)


def _rel_err(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def _teacher_forced_both(ours, rm, n_decode=24):
    """Prompt in batches of 8 (the reference's n_batch), then n_decode single-token decode steps
    fed from the reference's argmax; per step: max rel logit error, fraction of identical bits."""
    toks = ours.tokenize(PROMPT)
    n_past = 0
    errs, same = [], []
    for i in range(0, len(toks), 8):
        chunk = toks[i:i + 8]
        a = ours.eval(n_past, chunk, all_logits=True)
        b = rm.eval(n_past, chunk, all_logits=True)
        errs.append(_rel_err(a, b))
        same.append(float(np.mean(a == b)))
        n_past += len(chunk)
    nxt = int(np.argmax(b[-1]))
    for _ in range(n_decode):
        a = ours.eval(n_past, [nxt])
        b = rm.eval(n_past, [nxt])
        errs.append(_rel_err(a, b))
        same.append(float(np.mean(a == b)))
        n_past += 1
        nxt = int(np.argmax(b[-1]))
    print("max rel logit error per step:", ["%.2e" % e for e in errs])
    print("fraction of bit-identical logits per step:", ["%.4f" % f for f in same])
    return errs, same


def _gpu_vs_ref(path, check):
    lib = G.runtime()
    be = G.mi355x_backend(lib)
    ours = gpt2.Model(lib, path, be, n_ctx=1024, n_batch=8)
    ref, rbe, rm = _ref_model(path)
    try:
        check(ours, rm)
    finally:
        ours.free()
        rm.free()
        lib.ggml_backend_free(be)
        ref.ggml_backend_free(rbe)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
def test_gpt2_logits_match_reference_cpu(model_path):
    """Teacher-forced f16 model, default (fast, tree-order) decode GEMVs: every step's logits
    within the north_star's 1e-3 of the reference CPU's."""
    def check(ours, rm):
        errs, _ = _teacher_forced_both(ours, rm)
        assert max(errs) <= LOGIT_TOL, errs
    _gpu_vs_ref(model_path, check)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
def test_gpt2_logits_bit_identical_reference_order(model_path):
    """The same with mmv_order=1 (decode GEMVs in the reference CPU's summation order): every
    decode-path step's logits are the reference CPU's bits."""
    lib = G.runtime()
    assert lib.ggml_backend_mi355x_set_tuning(b"mmv_order", 1)
    try:
        def check(ours, rm):
            errs, same = _teacher_forced_both(ours, rm)
            assert max(errs) <= LOGIT_TOL, errs
            assert min(same) == 1.0, "decode-path logits are expected to be bit-identical to the CPU's"
        _gpu_vs_ref(model_path, check)
    finally:
        lib.ggml_backend_mi355x_set_tuning(b"mmv_order", -1)


# ---- quantized GPT-2 (examples/gpt-2/quantize.cpp): the north_star weight types end to end --------

QTYPES = ["q4_0", "q8_0", "q4_k", "q5_k"]
REF_QUANTIZE = os.path.join(REF, "gpt-2-quantize")


@pytest.fixture(scope="module")
def quantized_paths(model_path):
    lib = G.runtime()
    return {q: gpt2.ensure_quantized_model(lib, q) for q in QTYPES}


@pytest.mark.skipif(not os.path.exists(REF_QUANTIZE), reason="make -C oracle gpt2")
@pytest.mark.parametrize("qtype", QTYPES)
def test_quantize_model_matches_reference_program(model_path, tmp_path, qtype):
    """gpt2.quantize_model (our runtime's ggml_quantize_chunk) writes the same bytes as the
    reference's examples/gpt-2/quantize.cpp run on the same f16 model."""
    import filecmp
    ours = gpt2.quantize_model(G.runtime(), model_path, str(tmp_path / "ours.bin"), qtype)
    ref = str(tmp_path / "ref.bin")
    p = subprocess.run([REF_QUANTIZE, model_path, ref, qtype], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert os.path.getsize(ours) == os.path.getsize(ref)
    assert filecmp.cmp(ours, ref, shallow=False)


@pytest.mark.skipif(not (os.path.exists(REF_BIN) and os.path.exists(OUR_REF_BIN)), reason="make -C oracle gpt2")
def test_driver_matches_reference_program_q4_k(quantized_paths):
    """The quantized model through the reference program and our driver (reference CPU ops)."""
    args = ["-m", quantized_paths["q4_k"], "-p", PROMPT, "-n", "16", "-s", "5", "-t", "4"]
    ref = subprocess.run([REF_BIN] + args, capture_output=True, text=True, timeout=300)
    ours = subprocess.run([OUR_REF_BIN] + args, capture_output=True, text=True, timeout=300)
    assert ref.returncode == 0 and ours.returncode == 0, (ref.stderr[-1000:], ours.stderr[-1000:])
    assert _text(ref.stdout) == _text(ours.stdout)


@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
def test_reference_quantized_gpt2_is_ulp_sensitive(quantized_paths):
    """Why quantized GPT-2 parity is checked bit for bit (mmv_order=1) and not against 1e-3: the
    reference's own logits move by ~1e-2 when one input is perturbed by 1 ulp, because every
    layer re-quantizes its activations (round(x / d) jumps a whole step at a rounding boundary).
    Measured on the reference CPU alone: 1-ulp change of every model/wpe value."""
    src = quantized_paths["q4_0"]
    data = bytearray(open(src, "rb").read())
    off = data.index(b"model/wpe") + len(b"model/wpe")
    n = 768 * 1024
    wpe = np.frombuffer(data, dtype=np.uint32, count=n, offset=off).copy() ^ 1
    data[off:off + 4 * n] = wpe.tobytes()
    pert = src + ".ulp.bin"
    open(pert, "wb").write(data)
    outs = []
    try:
        for p in (src, pert):
            ref, be, m = _ref_model(p)
            try:
                outs.append(m.eval(0, m.tokenize(PROMPT)[:8], all_logits=True))
            finally:
                m.free()
                ref.ggml_backend_free(be)
    finally:
        os.remove(pert)
    print(f"reference q4_0 GPT-2: 1-ulp wpe perturbation moves the logits by {_rel_err(outs[1], outs[0]):.2e}")
    assert _rel_err(outs[1], outs[0]) > 10 * LOGIT_TOL


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
@pytest.mark.parametrize("qtype", QTYPES)
def test_quantized_gpt2_logits_bit_identical_to_reference_cpu(quantized_paths, qtype):
    """Teacher-forced quantized model on MI355X (quantized get_rows embedding, quantized MUL_MAT for
    every projection and the lm_head) with the backend's DEFAULT settings (mmv_order -1: a graph
    whose quantized mul_mats consume computed activations runs its decode reductions in the
    reference's order): every step's logits are the reference CPU's bits. The explicit tree order
    (mmv_order=0): test_quantized_gpt2_tree_order_close_to_reference_cpu."""
    def check(ours, rm):
        errs, same = _teacher_forced_both(ours, rm, n_decode=12)
        assert min(same) == 1.0, (errs, same)
    _gpu_vs_ref(quantized_paths[qtype], check)


def _teacher_forced_prompt(ours, rm, n_batch, n_decode=4):
    """A repeated PROMPT (> 64 tokens, and longer than one n_batch chunk) in chunks of n_batch (so
    prompt mul_mats have up to n_batch columns), then a few decode steps; returns per-step max rel
    error and bit-identical fraction."""
    reps = 3
    toks = ours.tokenize(" ".join([PROMPT] * reps))
    while len(toks) <= n_batch + 16:
        reps += 3
        toks = ours.tokenize(" ".join([PROMPT] * reps))
    assert len(toks) > 64
    n_past, errs, same = 0, [], []
    for i in range(0, len(toks), n_batch):
        chunk = toks[i:i + n_batch]
        a = ours.eval(n_past, chunk, all_logits=True)
        b = rm.eval(n_past, chunk, all_logits=True)
        errs.append(_rel_err(a, b))
        same.append(float(np.mean(a == b)))
        n_past += len(chunk)
    nxt = int(np.argmax(b[-1]))
    for _ in range(n_decode):
        a = ours.eval(n_past, [nxt])
        b = rm.eval(n_past, [nxt])
        errs.append(_rel_err(a, b))
        same.append(float(np.mean(a == b)))
        n_past += 1
        nxt = int(np.argmax(b[-1]))
    print(f"n_batch {n_batch}: max rel logit error per step", ["%.2e" % e for e in errs])
    print(f"n_batch {n_batch}: bit-identical fraction per step", ["%.4f" % f for f in same])
    return errs, same


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
@pytest.mark.parametrize("qtype", ["q4_k", "q4_0"])
@pytest.mark.parametrize("n_batch", [32, 64, 128, 512])
def test_quantized_gpt2_prompt_path_bit_identical_to_reference_cpu(quantized_paths, qtype, n_batch):
    """The quantized model's PROMPT path: prompts evaluated in chunks of 32 .. 512 tokens (both sides
    the same batching), so every projection is a mul_mat of up to n_batch columns. With the default
    settings such a graph runs in the reference order (mmv_order -1 -> 1), and its quantized prompt
    mul_mats -- of any column count since round 6 -- take the reference-order streaming GEMV, 8
    columns per grouped member, instead of the MFMA GEMM (ord_prefill_cols): every prompt and decode
    step's logits are the reference CPU's bits."""
    lib = G.runtime()
    be = G.mi355x_backend(lib)
    ours = gpt2.Model(lib, quantized_paths[qtype], be, n_ctx=1024, n_batch=n_batch)
    ref, rbe, rm = _ref_model_nb(quantized_paths[qtype], n_batch)
    try:
        errs, same = _teacher_forced_prompt(ours, rm, n_batch)
        assert min(same) == 1.0, (errs, same)
    finally:
        ours.free()
        rm.free()
        lib.ggml_backend_free(be)
        ref.ggml_backend_free(rbe)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
@pytest.mark.parametrize("qtype", ["q4_k", "q4_0"])
def test_quantized_gpt2_mfma_prompt_path_deviation(quantized_paths, qtype):
    """The same prompt through the exact int8-MFMA prefill GEMMs (ord_prefill_cols 0: the opt-out
    from the reference-order prompt path): exact integer block sums, own f32 fold order; the logits
    then differ from the reference CPU's by the model's re-quantization sensitivity -- recorded
    here beside the reference's own 1-ulp sensitivity (1.7e-2 of max|logit|,
    test_reference_quantized_gpt2_is_ulp_sensitive) and bounded by the same 3e-2 as the tree-order
    decode (test_quantized_gpt2_tree_order_close_to_reference_cpu)."""
    lib = G.runtime()
    assert lib.ggml_backend_mi355x_set_tuning(b"ord_prefill_cols", 0)
    be = G.mi355x_backend(lib)
    ours = gpt2.Model(lib, quantized_paths[qtype], be, n_ctx=1024, n_batch=64)
    ref, rbe, rm = _ref_model_nb(quantized_paths[qtype], 64)
    try:
        errs, _ = _teacher_forced_prompt(ours, rm, 64)
        print(f"{qtype}: MFMA prompt path max rel logit error {max(errs):.3e}")
        assert max(errs) <= 3e-2, errs
    finally:
        lib.ggml_backend_mi355x_set_tuning(b"ord_prefill_cols", 2 ** 31 - 1)
        ours.free()
        rm.free()
        lib.ggml_backend_free(be)
        ref.ggml_backend_free(rbe)


@pytest.mark.gpu
@pytest.mark.parametrize("qtype", ["f16", "q4_k", "q8_0"])
@pytest.mark.parametrize("order", [-1, 0, 1])
def test_gpt2_decode_launches_per_token(model_path, quantized_paths, qtype, order):
    """Node fusion keeps a decode token at 62 kernel launches for f16 and quantized models alike:
    per layer the norm chain rides in the GEMV prologue, bias / residual / GELU and the K/V-cache
    copies in its epilogue, the attention block is one kernel; the token + position embedding
    (two GET_ROWS and their ADD) is one kernel. The f16 model in the tree-order (default) mode
    also runs each layer's attention with its output projection (k_attn_proj, partial sums added
    by the next GEMV's norm prologue): 50."""
    lib = G.runtime()
    be = G.mi355x_backend(lib)
    lib.ggml_backend_mi355x_set_tuning(b"mmv_order", order)
    m = gpt2.Model(lib, model_path if qtype == "f16" else quantized_paths[qtype], be, n_ctx=1024, n_batch=8)
    try:
        toks = m.tokenize(PROMPT)
        m.eval(0, toks[:8])
        m.eval(8, [toks[8]])
        assert lib.ggml_backend_mi355x_last_launch_count(be) == (50 if qtype == "f16" and order <= 0 else 62)
    finally:
        lib.ggml_backend_mi355x_set_tuning(b"mmv_order", -1)
        m.free()
        lib.ggml_backend_free(be)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
@pytest.mark.parametrize("qtype", QTYPES)
def test_quantized_gpt2_tree_order_close_to_reference_cpu(quantized_paths, qtype):
    """mmv_order=0 (tree order forced) on the quantized models: per-op error is f32 summation order
    only (<= 1e-5, test_mul_mat_gpu), amplified by the model's activation re-quantization to the
    reference's own 1-ulp sensitivity (1.7e-2, test_reference_quantized_gpt2_is_ulp_sensitive).
    Measured on MI355X (profiles/r03o_gpt2_default_order.txt): q4_0 1.4e-2, q8_0 1.6e-2, q4_k 2.1e-2,
    q5_k 2.1e-2 of max|logit|; bound 3e-2. This is why the default picks the reference order for
    such graphs (test above)."""
    lib = G.runtime()
    assert lib.ggml_backend_mi355x_set_tuning(b"mmv_order", 0)
    try:
        def check(ours, rm):
            errs, _ = _teacher_forced_both(ours, rm, n_decode=12)
            print(f"{qtype}: tree order max rel logit error {max(errs):.3e}")
            assert max(errs) <= 3e-2, errs
        _gpu_vs_ref(quantized_paths[qtype], check)
    finally:
        lib.ggml_backend_mi355x_set_tuning(b"mmv_order", -1)


@pytest.mark.gpu
def test_gpt2_cli_on_mi355x(model_path):
    """The product CLI (-ngl 100 runs the whole graph on MI355X) generates and reports timing."""
    p = subprocess.run([OUR_BIN, "-m", model_path, "-p", PROMPT, "-n", "32", "-s", "7", "-ngl", "100"],
                       capture_output=True, text=True, timeout=300)
    print(p.stdout[-1500:], p.stderr[-1500:])
    assert p.returncode == 0
    assert "using MI355X0 backend" in p.stderr
    assert "per token" in p.stdout


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="make -C oracle gpt2")
def test_gpt2_cli_on_mi355x_samples_reference_text(model_path):
    """Seeded sampling on MI355X (-ngl 100, GGML_MI355X_MMV_ORDER=1) prints the same text as the
    reference program (examples/gpt-2/main-backend.cpp) on the reference CPU: the logits are
    bit-identical."""
    args = ["-m", model_path, "-p", PROMPT, "-n", "48", "-s", "11", "-t", "8"]
    ref = subprocess.run([REF_BIN] + args, capture_output=True, text=True, timeout=300)
    ours = subprocess.run([OUR_BIN] + args + ["-ngl", "100"], capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, GGML_MI355X_MMV_ORDER="1"))
    assert ref.returncode == 0 and ours.returncode == 0, (ref.stderr[-1000:], ours.stderr[-1000:])
    print(_text(ours.stdout))
    assert _text(ours.stdout) == _text(ref.stdout)


@pytest.mark.gpu
def test_gpt2_long_context_decode(model_path):
    """Positions up to the 1024-token context: attention over long KV (strided f32 mul_mats,
    soft_max rows of 1000+) stays finite and close to the reference at the last step."""
    lib = G.runtime()
    be = G.mi355x_backend(lib)
    ours = gpt2.Model(lib, model_path, be, n_ctx=1024, n_batch=512)
    ref, rbe, rm = _ref_model(model_path)
    try:
        rng = np.random.default_rng(3)
        toks = rng.integers(0, 50257, size=1000).astype(np.int32)
        a = ours.eval(0, toks[:512], all_logits=False)
        b = rm.eval(0, toks[:512], all_logits=False)
        e1 = _rel_err(a, b)
        a = ours.eval(512, toks[512:1000], all_logits=False)
        b = rm.eval(512, toks[512:1000], all_logits=False)
        e2 = _rel_err(a, b)
        # single-token decode at n_kv > 1000 (the fused attention + projection path, long KV)
        e3 = []
        for k in range(3):
            nxt = [int(np.argmax(b[-1]))]
            a = ours.eval(1000 + k, nxt)
            b = rm.eval(1000 + k, nxt)
            e3.append(_rel_err(a, b))
        print(f"long context: rel logit error {e1:.2e} (512-token prompt), {e2:.2e} (488 more), decode {e3}")
        assert np.isfinite(a).all()
        assert e1 <= LOGIT_TOL and e2 <= LOGIT_TOL and max(e3) <= LOGIT_TOL
        with pytest.raises(RuntimeError):
            ours.eval(1003, toks[:100])  # past the 1024 positions of wpe
    finally:
        ours.free()
        rm.free()
        lib.ggml_backend_free(be)
        ref.ggml_backend_free(rbe)


@pytest.mark.gpu
def test_gpt2_decode_to_context_end_then_restart(model_path):
    """Decode single tokens up to the last KV slot (where no next-step plan can be prebuilt), then
    restart from position 0 and repeat, then free: every prebuilt graph plan is freed exactly once
    (a plan taken by the fast path is owned by that eval), and the second pass reproduces the first
    pass's logits bit for bit."""
    lib = G.runtime()
    be = G.mi355x_backend(lib)
    n_ctx = 24
    m = gpt2.Model(lib, model_path, be, n_ctx=n_ctx, n_batch=8)
    try:
        toks = m.tokenize(PROMPT)[:8]
        passes = []
        for _ in range(2):
            outs = [m.eval(0, toks)]
            n_past, nxt = len(toks), int(np.argmax(outs[-1][-1]))
            while n_past < n_ctx:
                outs.append(m.eval(n_past, [nxt]))
                n_past += 1
                nxt = int(np.argmax(outs[-1][-1]))
            passes.append(np.concatenate(outs))
        assert np.isfinite(passes[0]).all()
        assert np.array_equal(passes[0].view(np.uint32), passes[1].view(np.uint32))
        with pytest.raises(RuntimeError):
            m.eval(n_ctx, [0])  # past the KV cache
    finally:
        m.free()
        lib.ggml_backend_free(be)


# ---- ggml_backend_sched: the backend as a drop-in under the reference scheduler -------------------

SCHED_CHILD = os.path.join(REPO, "tests", "_sched_child.py")


def _teacher_forced_direct(m, toks):
    outs, n_past = [], 0
    for i in range(0, len(toks), 8):
        outs.append(m.eval(n_past, toks[i:i + 8], all_logits=True))
        n_past += len(toks[i:i + 8])
    nxt = int(np.argmax(outs[-1][-1]))
    for _ in range(8):
        lg = m.eval(n_past, [nxt])
        outs.append(lg)
        n_past += 1
        nxt = int(np.argmax(lg[-1]))
    return np.concatenate(outs)


def _run_sched_child(model_path, tmp_path, layers, order="1"):
    """order "1": the MI355X layers' decode GEMVs in the reference order (bit-identical splits);
    None: the backend's default (per graph, csrc/backend/graph.cpp graph_decode_order)."""
    import sys
    env = dict(os.environ)
    env.pop("GGML_MI355X_MMV_ORDER", None)
    if order is not None:
        env["GGML_MI355X_MMV_ORDER"] = order
    p = subprocess.run([sys.executable, SCHED_CHILD, model_path, str(tmp_path), ",".join(str(v) for v in layers)],
                       capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
def test_sched_mode_on_reference_cpu_matches_direct(model_path, tmp_path):
    """main-sched.cpp's path (ggml_backend_sched, CPU only) == main-backend.cpp's path, bit for bit."""
    _run_sched_child(model_path, tmp_path, [0])
    ref, be, m = _ref_model(model_path)
    try:
        direct = _teacher_forced_direct(m, m.tokenize(PROMPT))
    finally:
        m.free()
        ref.ggml_backend_free(be)
    sched = np.load(tmp_path / "ngl0.npy")
    assert np.array_equal(sched.view(np.uint32), direct.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
def test_gpt2_partial_offload_under_reference_scheduler(model_path, tmp_path):
    """examples/gpt-2/main-sched.cpp's layer split: the reference's own ggml_backend_sched places
    n_gpu_layers of 12 on MI355X0 and the rest on the reference CPU backend, copying activations
    across the split. Every split point gives logits bit-identical to the CPU-only run."""
    out = _run_sched_child(model_path, tmp_path, [0, 3, 6, 12, 13])
    print(out)
    base = np.load(tmp_path / "ngl0.npy")
    for ngl in (3, 6, 12, 13):
        got = np.load(tmp_path / f"ngl{ngl}.npy")
        diff = float(np.max(np.abs(got - base)))
        print(f"n_gpu_layers={ngl}: max |d| = {diff:.3e}")
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), (ngl, diff)
    import re
    splits = {int(a): int(b) for a, b in re.findall(r"n_gpu_layers=(\d+): splits=(\d+)", out)}
    assert splits[6] > 1 and splits[3] > 1  # the graph really crosses devices


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
def test_gpt2_scheduler_options_host_inputs_events_mid_layer_split(model_path, tmp_path):
    """The rest of the scheduler contract: the pinned host buffer type holding the persistent
    inputs (its supports_backend delegates to the CPU buffer type, ggml-cuda.cu:1037-1038),
    parallel=true (input copies + the backend event vtable, ggml-backend.c:1647-1710) and a split
    boundary inside a layer (attention on MI355X0, MLP on the CPU), where a tensor read by both
    splits must be stored by the first. Logits bit-identical to the CPU-only run."""
    specs = ["0", "6:0:h", "6:1", "6:1:h", "6:2", "12:1:h"]
    out = _run_sched_child(model_path, tmp_path, specs)
    print(out)
    base = np.load(tmp_path / "ngl0.npy")
    for spec in specs[1:]:
        got = np.load(tmp_path / ("ngl" + spec.replace(":", "_") + ".npy"))
        diff = float(np.max(np.abs(got - base)))
        print(f"{spec}: max |d| = {diff:.3e}")
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), (spec, diff)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
def test_gpt2_partial_offload_default_order(model_path, tmp_path):
    """The same scheduler splits with the backend's DEFAULT settings (no GGML_MI355X_MMV_ORDER):
    the f16 model's graphs keep the tree order, so every split is within the north_star's 1e-3
    (of max |logit|) of the CPU-only run, a mid-layer split included."""
    specs = ["0", "3", "6", "12", "6:2"]
    out = _run_sched_child(model_path, tmp_path, specs, order=None)
    print(out)
    base = np.load(tmp_path / "ngl0.npy")
    scale = float(np.max(np.abs(base)))
    for spec in specs[1:]:
        got = np.load(tmp_path / ("ngl" + spec.replace(":", "_") + ".npy"))
        rel = float(np.max(np.abs(got - base))) / scale
        print(f"{spec}: max |d| / max |logit| = {rel:.3e}")
        assert rel <= 1e-3, (spec, rel)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
def test_quantized_gpt2_partial_offload_default_order_bit_identical(quantized_paths, tmp_path):
    """A Q4_K model under the reference scheduler with the DEFAULT settings: the scheduler's split
    inputs are fresh NONE tensors named "<backend>#<src>#<copy>" (ggml-backend.c:1498-1523) that
    hold computed activations, so graph_decode_order must run those graphs in the reference order.
    Every split, a mid-layer one included, is bit-identical to the CPU-only run."""
    specs = ["0", "3", "6", "12", "6:2"]
    out = _run_sched_child(quantized_paths["q4_k"], tmp_path, specs, order=None)
    print(out)
    base = np.load(tmp_path / "ngl0.npy")
    for spec in specs[1:]:
        got = np.load(tmp_path / ("ngl" + spec.replace(":", "_") + ".npy"))
        diff = float(np.max(np.abs(got - base)))
        print(f"{spec}: max |d| = {diff:.3e}")
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), (spec, diff)


# ---- batched independent sequences (examples/gpt-2/main-batched.cpp) ---------------------------------

def _batched_scenario(n_parallel, steps=6, seed=11):
    """An 8-token prompt (one decode-path batch) shared by every sequence, then `steps` batches of
    one token per sequence, the tokens drawn per sequence so the sequences diverge."""
    rng = np.random.default_rng(seed + n_parallel)
    return rng.integers(0, 50257, size=(steps, n_parallel)).tolist()


@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
def test_batched_sequences_match_single_sequence_runs_on_reference_cpu(model_path):
    """The driver's batched mode (KV cells + seq ids + main-batched's KQ mask, run on the reference
    CPU ops) gives every sequence the logits of that sequence run alone through main-backend's
    graph: the cell bookkeeping and the mask are right (different graphs: close, not bit-equal)."""
    ref, be, m = _ref_model(model_path)
    try:
        prompt = m.tokenize(PROMPT)[:8]
        npar, forced = 3, _batched_scenario(3, steps=4)
        b = gpt2.run_batched(m, prompt, npar, forced)
        for s in range(npar):
            toks = prompt + [forced[t][s] for t in range(len(forced))]
            want = m.eval(0, toks, all_logits=True)[len(prompt) - 1:]
            got = np.stack([b[0]] + [b[1 + t * npar + s] for t in range(len(forced))])
            assert _rel_err(got, want) <= 1e-3, (s, _rel_err(got, want))
    finally:
        m.free()
        ref.ggml_backend_free(be)


def _batched_gpu_vs_ref(model_path, n_parallel):
    lib = G.runtime()
    be = G.mi355x_backend(lib)
    ours = gpt2.Model(lib, model_path, be, n_ctx=256, n_batch=8)
    ref, rbe, rm = _ref_model(model_path)
    try:
        prompt = ours.tokenize(PROMPT)[:8]
        forced = _batched_scenario(n_parallel)
        a = gpt2.run_batched(ours, prompt, n_parallel, forced)
        b = gpt2.run_batched(rm, prompt, n_parallel, forced)
        return a, b
    finally:
        ours.free()
        rm.free()
        lib.ggml_backend_free(be)
        ref.ggml_backend_free(rbe)


@pytest.mark.gpu
def test_batched_logits_in_place_equal_copied(model_path):
    """decode_batch(copy=False) -- the logits read in place from the pinned staging, as the batched
    bench's loop does -- returns the same bits as the copied logits, step after step (the view of
    one step is consumed before the next call overwrites the staging)."""
    lib = G.runtime()
    be = G.mi355x_backend(lib)
    ours = gpt2.Model(lib, model_path, be, n_ctx=256, n_batch=8)
    try:
        prompt = ours.tokenize(PROMPT)[:8]
        forced = _batched_scenario(8)
        a = gpt2.run_batched(ours, prompt, 8, forced, copy=True)
        b = gpt2.run_batched(ours, prompt, 8, forced, copy=False)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        ours.free()
        lib.ggml_backend_free(be)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
@pytest.mark.parametrize("n_parallel", [2, 4, 8])
def test_batched_sequences_match_reference_cpu(model_path, n_parallel):
    """main-batched.cpp's flow (shared prompt, n_parallel sequences decoded together) on MI355X with
    the default settings: every batch's logits within 1e-3 of max |logit| of the reference CPU
    running the same driver and graph."""
    a, b = _batched_gpu_vs_ref(model_path, n_parallel)
    err = _rel_err(a, b)
    print(f"n_parallel={n_parallel}: max rel logit error {err:.2e}")
    assert err <= LOGIT_TOL


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
@pytest.mark.parametrize("n_parallel", [2, 4, 8])
def test_batched_sequences_bit_identical_reference_order(model_path, n_parallel):
    """The same with mmv_order=1: every batch (at most 8 tokens: the decode path) bit-identical to the
    reference CPU's logits."""
    lib = G.runtime()
    assert lib.ggml_backend_mi355x_set_tuning(b"mmv_order", 1)
    try:
        a, b = _batched_gpu_vs_ref(model_path, n_parallel)
    finally:
        lib.ggml_backend_mi355x_set_tuning(b"mmv_order", -1)
    print(f"n_parallel={n_parallel}: identical {float(np.mean(a == b)):.4f}, max rel err {_rel_err(a, b):.2e}")
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
