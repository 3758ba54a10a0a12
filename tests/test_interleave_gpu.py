"""`-m gpu`: interleaved text-and-image generation -- the two kernels of csrc/interleave.hip against their restatements
(tests/interleave_ref.py), and `generate_interleaved` on a TINY model whose lm_head is edited so that greedy decoding emits
<dream_start> (and, for the ragged batch, an eos id) at a known step."""
import pytest
import torch

import interleave_ref as R
from conftest import check_tensor, rel_l2
from sampling_ref import reference_sample

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
MEAN, STD = [0.48145466, 0.4578275, 0.40821073], [0.26862954, 0.26130258, 0.27577711]


# ------------------------------------------------------------------------------------------------------------ park kernel
def _park_case(B):
    """5 steps of tokens for B rows (eos 2, trigger 9): row 0 runs, row 1 was parked before, row 2 chooses eos at step 1, row 3 the
    trigger at step 1 (eos and trigger in one step on different rows), row 4 the trigger at step 3, row 5 eos then the trigger (stays 1)."""
    toks = torch.randint(10, 100, (5, B), generator=torch.Generator().manual_seed(B))
    plan = {2: [(1, 2)], 3: [(1, 9)], 4: [(3, 9), (4, 2)], 5: [(0, 2), (2, 9)], 6: [(4, 9)], 7: [(2, 2)]}
    for b, events in plan.items():
        if b < B:
            for s, t in events:
                toks[s, b] = t
    if B == 1:
        toks[2, 0] = 9
    parked = [0] * B
    if B > 1:
        parked[1] = 2
    return toks, parked


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_park_kernel_matches_restatement(B, mode):
    from dreamllm_amd import ops
    toks, parked0 = _park_case(B)
    ref = dict(parked=list(parked0), park_step=[7 if p else 0 for p in parked0], pos=[20 + 3 * b for b in range(B)],
               kv_len=[25 + b for b in range(B)], slot=[100 * b + 24 for b in range(B)])
    dev = {k: torch.tensor(v, dtype=torch.int32 if k in ("parked", "kv_len") else torch.long, device=DEV) for k, v in ref.items()}
    tok = torch.zeros(B, dtype=torch.long, device=DEV)
    step = torch.full((1,), 10, dtype=torch.long, device=DEV)
    toks_d = toks.to(DEV)
    idx = torch.zeros(1, dtype=torch.long, device=DEV)

    def one():  # what a captured token step does around the launch: the token comes from device memory, the counter advances first
        tok.copy_(toks_d.index_select(0, idx)[0])
        step.add_(1)
        ops.interleave_park(tok, dev["parked"], dev["park_step"], step, eos=2, trigger=9, pos=dev["pos"], kv_len=dev["kv_len"],
                            slot=dev["slot"])
        idx.add_(1)

    graph = None
    if mode == "graph":
        keep = {k: v.clone() for k, v in dev.items()}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            one()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            one()
        for k, v in keep.items():
            dev[k].copy_(v)
        idx.zero_()
        step.fill_(10)
    for s in range(5):
        graph.replay() if graph is not None else one()
        R.park_ref(toks[s].tolist(), 2, 9, 11 + s, ref["parked"], ref["park_step"], ref["pos"], ref["kv_len"], ref["slot"])
        for k in ref:
            assert dev[k].cpu().tolist() == ref[k], (B, mode, s, k)
    assert any(ref["parked"]) and (B == 1 or 0 in ref["parked"])
    # the first token of a phase: parks without advancing
    before = {k: dev[k].clone() for k in ("pos", "kv_len", "slot")}
    dev["parked"].zero_()
    tok.fill_(9)
    ops.interleave_park(tok, dev["parked"], dev["park_step"], step, eos=2, trigger=9)
    assert dev["parked"].cpu().tolist() == [2] * B and all(torch.equal(dev[k], v) for k, v in before.items())


# ---------------------------------------------------------------------------------------------------------- image hand-off
_SHAPES = [(64, 64), (96, 64), (67, 53), (64, 53)]   # (64, 53): odd rows that start off a 16-byte boundary, planes that do not
_SIZES = [14, 32, 224]
# Largest |torch(bf16-rounded input) - torch(fp32 input)| of the definition over the cases below, measured on the MI355X: the fp32
# output may differ from the definition by 2 x this (tap weights summed in another order).  Recomputed and printed by the test;
# the kernel's own largest difference from the definition on these cases was 5.8e-5 (64 x 64 -> 224).
BF16_INPUT_ERR_MEASURED = 9.0572e-03
# By how much two fp32 evaluations of the definition may differ (the bound of tests/test_interleave_cpu.py, derived there from the
# fp32 rounding of the tap centres: <= 1e-5 source pixels, cubic slope <= 1, 2 x 5 taps that matter, 1 / std ~ 3.8).  It does not
# come from the kernel under test.
FP32_RESOLUTION = 1e-4


def _hand_off_inputs(H, W, signed):
    g = torch.Generator().manual_seed(H * 131 + W)
    x = torch.rand(2, 3, H, W, generator=g) * 1.4 - 0.2
    return ((x * 2 - 1) if signed else x).to(DEV)


@pytest.fixture(scope="module")
def bf16_input_err():
    worst = 0.0
    for H, W in _SHAPES:
        for size in _SIZES:
            for signed in (False, True):
                x = _hand_off_inputs(H, W, signed)
                d = R.torch_hand_off(x.to(BF).float(), size, MEAN, STD, signed) - R.torch_hand_off(x, size, MEAN, STD, signed)
                worst = max(worst, float(d.abs().max()))
    print(f"torch bf16-input vs fp32-input hand-off: max abs difference {worst:.4e} (recorded: {BF16_INPUT_ERR_MEASURED:.4e})")
    return worst


@pytest.mark.parametrize("H,W", _SHAPES)
@pytest.mark.parametrize("size", _SIZES)
def test_image_to_clip_matches_torch(H, W, size, bf16_input_err):
    from dreamllm_amd import ops
    assert 1e-3 < bf16_input_err < 5e-2     # half a bf16 ulp of a value in [0.5, 1) is 2e-3; 1 / std ~ 3.8 and overshoot scale it
    for signed in (False, True):
        x = _hand_off_inputs(H, W, signed)
        ref = R.torch_hand_off(x, size, MEAN, STD, signed)
        got = ops.image_to_clip(x, size, MEAN, STD, out_dtype=torch.float32, signed_range=signed)
        assert got.shape == ref.shape == (2, 3, size, size) and bool(torch.isfinite(got).all())
        err = float((got - ref).abs().max())
        print(f"image_to_clip {H}x{W} -> {size} signed={signed}: max abs err {err:.3e} (bound {2 * bf16_input_err:.3e})")
        assert err <= 2 * bf16_input_err
        gb = ops.image_to_clip(x, size, MEAN, STD, out_dtype=BF, signed_range=signed)
        rb = ref.to(BF)
        assert gb.dtype == BF and bool(torch.isfinite(gb).all())
        # one bf16 ulp of the rounded reference -- or FP32_RESOLUTION where the ulp is finer than that: the outputs are differences
        # (v - mean) / std that cross zero, where the ulp of the value shrinks without limit while two fp32 evaluations of the
        # definition differ by an ABSOLUTE amount
        ulp = rb.float().abs().clamp_min(2.0 ** -126).log2().floor().exp2() * 2.0 ** -7
        assert bool(((gb.float() - rb.float()).abs() <= ulp.clamp_min(FP32_RESOLUTION)).all())
        # bf16 input (what a bf16 VAE hands over) is read as its exact fp32 value
        xb = x.to(BF)
        got_b = ops.image_to_clip(xb, size, MEAN, STD, out_dtype=torch.float32, signed_range=signed)
        assert float((got_b - R.torch_hand_off(xb.float(), size, MEAN, STD, signed)).abs().max()) <= 2 * bf16_input_err


def test_image_to_clip_in_a_graph_and_bad_arguments():
    from dreamllm_amd import ops
    x = _hand_off_inputs(96, 64, False)
    out = torch.empty(2, 3, 32, 32, dtype=BF, device=DEV)
    eager = ops.image_to_clip(x, 32, MEAN, STD, out_dtype=BF)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.image_to_clip(x, 32, MEAN, STD, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.image_to_clip(x, 32, MEAN, STD, out=out)
    out.zero_()
    graph.replay()
    assert torch.equal(out, eager)
    with pytest.raises(ValueError):
        ops.image_to_clip(x[:, :2], 32, MEAN, STD)
    with pytest.raises(ValueError):          # a 40-fold reduction does not fit the tile's tap storage
        ops.image_to_clip(torch.zeros(1, 3, 640, 640, device=DEV), 16, MEAN, STD)


# ------------------------------------------------------------------------------------------------------- generate_interleaved
S, N_NEW, IMG, STEPS, GUIDE = 12, 44, 64, 2, 3.0
EOS = 31990


@pytest.fixture(scope="module")
def world():
    """A TINY model with CLIP and SD parts; three prompts; lm_head edited so that row 0 emits <dream_start> at step j and row 2 emits
    EOS at step e; the B = 1 fast-path results of each prompt (computed once, shared)."""
    from dreamllm_amd.factory import TINY, TINY_CLIP, TINY_DIFFUSION, build_dreamllm
    from dreamllm_amd.generation import interleave_layout
    from dreamllm_amd.schedulers import DDIMScheduler
    model = build_dreamllm(TINY, device=DEV, dtype=BF, seed=0, clip=TINY_CLIP, diffusion=TINY_DIFFUSION, num_dream_queries=8).eval()
    lay = interleave_layout(model)
    ids = torch.randint(3, 30000, (3, S), generator=torch.Generator().manual_seed(21)).to(DEV)
    neg = torch.randint(3, 30000, (1, 5), generator=torch.Generator().manual_seed(22)).to(DEV)
    j, tok_c = R.fire_step(model, ids[:1], lay.trigger)
    e, _ = R.fire_step(model, ids[2:3], EOS, lo=1)
    w = dict(model=model, lay=lay, ids=ids, neg=neg, j=j, tok_c=tok_c, e=e, sched=DDIMScheduler())
    w["kw"] = dict(max_new_tokens=N_NEW, eos_token_id=EOS, negative_prompt_ids=neg, guidance_scale=GUIDE, num_inference_steps=STEPS,
                   height=IMG, width=IMG, scheduler=w["sched"])
    w["solo"] = [_run(w, ids[b:b + 1], 100 + b) for b in range(3)]
    return w


def _run(w, ids, seed, **over):
    kw = dict(w["kw"], **over)
    return w["model"].generate_interleaved(ids, generator=torch.Generator().manual_seed(seed), **kw)


def _check_layout(w, seq, positions, prompt, n_new=None):
    lay = w["lay"]
    assert torch.equal(seq[: prompt.numel()].cpu(), prompt.cpu())
    assert [i for i, t in enumerate(seq.tolist()) if t == lay.trigger] == positions
    for p in positions:
        assert seq[p + 1: p + 1 + lay.block_len].tolist() == lay.ids_after_trigger()
    assert seq.numel() - prompt.numel() <= (N_NEW if n_new is None else n_new)


def test_structure_single_row(world):
    w = world
    out, lay, j = w["solo"][0], w["lay"], w["j"]
    assert len(out.sequences) == len(out.images) == len(out.image_positions) == 1
    seq = out.sequences[0]
    assert seq.dtype == torch.long and seq.dim() == 1
    _check_layout(w, seq, out.image_positions[0], w["ids"][0])
    assert out.image_positions == [[S + j]] and len(out.images[0]) == 1
    assert lay.ids_after_trigger()[: lay.n_query] == [lay.im_patch] * lay.n_query            # the builder's placeholder id
    for im in out.images[0]:
        assert im.shape == (3, IMG, IMG) and im.dtype == torch.float32 and float(im.min()) >= 0 and float(im.max()) <= 1
    assert seq.numel() > S + j + 1 + lay.block_len                                           # it carried on writing after <im_end>


def _recorded_call(w, ids, seed, **over):
    """A call on the cached session with every graph replay and phase opening recorded: [(phase, logits [B, V], tokens [B])]."""
    sess = w["model"]._decode_session[1]
    log, phase = [], [0]
    gen, begin = sess.generate, sess.begin_phase

    def generate(m):
        outs = []
        for _ in range(m):
            t = gen(1)
            log.append((phase[0], sess.logits.clone(), t[:, 0].clone()))
            outs.append(t)
        return torch.cat(outs, 1)

    def begin_phase(logits, p):
        phase[0] = p
        t = begin(logits, p)
        log.append((p, sess.first_logits.clone(), t.clone()))
        return t

    sess.generate, sess.begin_phase = generate, begin_phase
    try:
        out = _run(w, ids, seed, **over)
    finally:
        del sess.generate, sess.begin_phase
    assert w["model"]._decode_session[1] is sess, "the second call must reuse the cached session"
    return out, log, sess


def _decidable_tokens(log, b, phase, V):
    """Per recorded step of `phase`: (token emitted, reference greedy sample of that step's logits or None if undecidable)."""
    res = []
    for p, logits, tok in log:
        if p == phase:
            _, t, _, und = reference_sample(logits[b].float().cpu(), 1.0, 1, 1.0, V, 0.0)
            res.append((int(tok[b]), None if und else t))
    return res


def _agree(w, a, s, positions, log, b, prompt_len=None):
    """Sequences a (from the run `log` recorded, row b, images at `positions`) and s are equal, or their first difference sits on a
    step that fp32 cannot decide (a near-tie of the two largest logits)."""
    lay, V = w["lay"], w["model"].config.vocab_size
    a, s = list(a), list(s)
    n = min(len(a), len(s))
    diff = [i for i in range(n) if a[i] != s[i]]
    if diff or len(a) != len(s):
        i = diff[0] if diff else n
        cuts = [p + 1 + lay.block_len for p in positions if p + lay.block_len < i]
        phase, step = len(cuts), i - (cuts[-1] if cuts else (S if prompt_len is None else prompt_len))
        tok, ref = _decidable_tokens(log, b, phase, V)[step]
        assert ref is None, (b, i, tok, ref)


def _call_seed(seed):
    """The Philox seed `generate_interleaved` draws from `torch.Generator().manual_seed(seed)`."""
    from dreamllm_amd.modeling_dreamllm import DreamLLMForCausalMLM
    return DreamLLMForCausalMLM._draw_seed(torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def plain(world):
    """One plain forward over row 0's returned document through <im_end>, dream-query and CLIP embeddings spliced in: the fp32 oracle
    (truth) and the oracle in bf16 (yard-stick) -- hidden states, K/V, and the image synthesised from either's query states with
    the call's own noise and scheduler."""
    from dreamllm_amd.generation import clip_pixels, image_generator
    from oracle import llm_ref
    w = world
    model, lay, out = w["model"], w["lay"], w["solo"][0]
    p0 = out.image_positions[0][0]
    end = p0 + 1 + lay.block_len
    doc = out.sequences[0][:end].cpu()[None]
    cd = R.oracle_cfg(model)
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items() if k.startswith("model.") or k.startswith("lm_head")}
    with torch.no_grad():
        feats = model.model.clip_vision_embedding(clip_pixels(model, out.images[0][0][None].to(DEV)))
    dq = model.model.dream_embedding()[0].float().cpu()
    emb = llm_ref.splice_inputs(doc, sd, cd, dream_queries=dq, image_features=feats.float().cpu())
    h32, kv32 = R.forward_kv(emb, sd, cd)
    h16, kv16 = R.forward_kv(emb.to(BF), {k: v.to(BF) for k, v in sd.items()}, cd)

    def synth(hidden):
        negative = model.get_prompt_embeds(w["neg"])
        return model.stable_diffusion_head.pipeline(height=IMG, width=IMG, num_inference_steps=STEPS, guidance_scale=GUIDE,
                                                    generator=image_generator(_call_seed(100), 0, 0), prompt_embeds=hidden.to(DEV),
                                                    negative_prompt_embeds=negative, output_type="pt", scheduler=w["sched"])[0]

    q0 = p0 + 1
    truth = synth(h32[:, q0:q0 + lay.n_query])
    yard = synth(h16[:, q0:q0 + lay.n_query].float())
    return dict(end=end, kv32=kv32, kv16=kv16, truth=truth, err_ref=rel_l2(yard, truth))


def test_replay_chain_and_cache(world, plain):
    """A second call with the same arguments: the cached session and graph, bit-identical sequences (7); after <im_end> every token
    is the reference sample of its step's logits (3); the session's K/V from the prompt through the last <im_end> match one plain
    forward over the assembled embeddings (4); the image equals the synthesis from a plain forward's hidden states (3)."""
    w = world
    model, lay, first = w["model"], w["lay"], w["solo"][0]
    _run(w, w["ids"][:1], 100)                                        # makes the B = 1 session the cached one
    graph_before = model._decode_session[1].graph
    out, log, sess = _recorded_call(w, w["ids"][:1], 100)
    assert sess.graph is graph_before and graph_before is not None
    assert torch.equal(out.sequences[0], first.sequences[0]) and out.image_positions == first.image_positions == [[S + w["j"]]]
    assert all(torch.equal(a, b) for a, b in zip(out.images[0], first.images[0]))
    seq, V = out.sequences[0], model.config.vocab_size
    # ---- the chain after the first <im_end>
    p0 = out.image_positions[0][0]
    after = seq[p0 + 1 + lay.block_len:].tolist()
    chain = _decidable_tokens(log, 0, 1, V)
    n_take = len(after)
    assert len(chain) >= n_take >= 1
    checked = skipped = 0
    for (tok, ref), want in zip(chain[:n_take], after[:n_take]):
        assert tok == want
        if ref is None:
            skipped += 1
        else:
            assert tok == ref
            checked += 1
    print(f"chain after <im_end>: {checked} decidable steps, {skipped} undecidable")
    assert checked >= 1 and checked >= 0.5 * n_take
    # ---- one plain forward over the assembled embeddings: fp32 oracle = truth, the oracle in bf16 = yard-stick
    end = plain["end"]
    for li, ((k32, v32), (k16, v16)) in enumerate(zip(plain["kv32"], plain["kv16"])):
        ours_k = sess.kc[li][0, :end].transpose(0, 1)[None]
        ours_v = sess.vc[li][0, :end].transpose(0, 1)[None]
        check_tensor(f"interleave_cache_k{li}", ours_k, k32, rel_l2(k16, k32))
        check_tensor(f"interleave_cache_v{li}", ours_v, v32, rel_l2(v16, v32))
    # ---- the image from the plain forward's hidden states at the query positions: same noise, same scheduler
    check_tensor("interleave_image", out.images[0][0], plain["truth"], plain["err_ref"])


def test_ragged_batch_and_ban(world):
    w = world
    lay, ids = w["lay"], w["ids"]
    out = _run(w, ids, 100)
    solo = w["solo"]
    assert solo[0].image_positions == [[S + w["j"]]] and len(solo[0].images[0]) == 1
    assert solo[1].image_positions[0] == [] and lay.trigger not in solo[1].sequences[0].tolist()   # row 1 never triggers
    s2 = solo[2].sequences[0].tolist()
    assert s2[-1] == EOS and s2.index(EOS) == S + w["e"] and len(s2) == S + w["e"] + 1              # row 2 ends at its eos
    for b in range(3):
        _check_layout(w, out.sequences[b], out.image_positions[b], ids[b])
        assert out.image_positions[b] == solo[b].image_positions[0], b
        assert len(out.images[b]) == len(solo[b].images[0])
    assert out.images[1] == [] and out.sequences[2].tolist() == s2
    # token agreement with the row alone wherever the step is decidable: the rows are compared step by step on a recorded run
    _, log, sess = _recorded_call(w, ids, 100)
    for b in range(3):
        _agree(w, out.sequences[b].tolist(), solo[b].sequences[0].tolist(), out.image_positions[b], log, b)
    banned = _run(w, ids, 100, max_images=0)
    assert all(lay.trigger not in s.tolist() for s in banned.sequences) and banned.images == [[], [], []]
    assert banned.image_positions == [[], [], []]


def test_paths_agree(world, plain):
    w = world
    slow = _run(w, w["ids"], 100, fast=False)
    fast = _run(w, w["ids"], 100)
    _, log, _ = _recorded_call(w, w["ids"], 100)
    for b in range(3):
        assert slow.image_positions[b] == fast.image_positions[b], b
        _check_layout(w, slow.sequences[b], slow.image_positions[b], w["ids"][b])
        _agree(w, fast.sequences[b].tolist(), slow.sequences[b].tolist(), fast.image_positions[b], log, b)
        assert len(slow.images[b]) == len(fast.images[b])
    # row 0's image: both paths draw the noise of (seed, row 0, image 0) and are held to the plain forward's image
    assert len(slow.images[0]) == len(fast.images[0]) == 1
    check_tensor("interleave_image_slow_path", slow.images[0][0], plain["truth"], plain["err_ref"])
    check_tensor("interleave_image_fast_path_batched", fast.images[0][0], plain["truth"], plain["err_ref"])


def test_left_padded_batch(world):
    """Rows of unequal length, LEFT-padded: row 0 is prompt 0 behind three pad tokens.  Its cache starts at slot 3 (`kv_start`), its
    positions at 0, and the block appends read its past as slots [3, cur): the document must be the one the unpadded row gives."""
    w = world
    lay, solo = w["lay"], w["solo"][0]
    pad = w["model"].config.pad_token_id
    long = torch.randint(3, 30000, (1, S + 3), generator=torch.Generator().manual_seed(23)).to(DEV)
    ids = torch.cat([torch.cat([torch.full((1, 3), pad, device=DEV), w["ids"][:1]], 1), long])
    am = torch.ones_like(ids)
    am[0, :3] = 0
    _run(w, ids, 100, attention_mask=am)
    out, log, sess = _recorded_call(w, ids, 100, attention_mask=am)
    assert torch.equal(out.sequences[0][:S], w["ids"][0]) and torch.equal(out.sequences[1][:S + 3], long[0])
    assert out.image_positions[0] == [S + w["j"]] and len(out.images[0]) == 1
    _check_layout(w, out.sequences[0], out.image_positions[0], w["ids"][0])
    _check_layout(w, out.sequences[1], out.image_positions[1], long[0])
    _agree(w, out.sequences[0].tolist(), solo.sequences[0].tolist(), out.image_positions[0], log, 0)
    assert int(sess.kv_start[0]) == 3 and int(sess.kv_start[1]) == 0


def test_second_image_and_budget(world):
    """Two images on one row (a second `begin_phase`, phase 2) and the ban of a used-up budget with max_images > 0.  Logits are
    linear in the lm_head row, so the step after the first image at which the trigger row wins again -- as it stands, or with the row
    of a later step's token added -- is known from the recorded logits of a run with the budget at one image."""
    w = world
    model, lay, j = w["model"], w["lay"], w["j"]
    ids, n_new, V = w["ids"][:1], 96, model.config.vocab_size
    _run(w, ids, 100, max_new_tokens=n_new, max_images=1)
    one, log, _ = _recorded_call(w, ids, 100, max_new_tokens=n_new, max_images=1)
    assert one.image_positions == [[S + j]] and len(one.images[0]) == 1
    ph = {p: [(lg[0].float().cpu(), int(t[0])) for q, lg, t in log if q == p] for p in (0, 1)}
    W, tok_c = model.lm_head.weight, w["tok_c"]            # the trigger row is 1.5 x row tok_c (the fixture's edit)
    saved = W[lay.trigger].clone()

    def wins(lg, tok_k):      # margin by which the row 1.5 x (row c [+ row k]) beats the step's maximum over the other ids
        rest = lg.clone()
        rest[lay.trigger] = float("-inf")
        return 1.5 * float(lg[tok_c] + (lg[tok_k] if tok_k is not None else 0.0)) - float(rest[:V].max())

    def first_win(tok_k, limit=14):
        """Step of phase 1 at which the row first wins, if phase 0 still fires at j alone and every step up to there is decided by
        more than 0.05 (bf16 noise)."""
        m0 = [wins(lg, tok_k) for lg, _ in ph[0][: j + 1]]
        if not (max(m0[:j], default=-1.0) < -0.05 and m0[j] > 0.05):
            return None
        for k, (lg, _) in enumerate(ph[1][:limit]):
            m = wins(lg, tok_k)
            if abs(m) <= 0.05:
                return None
            if m > 0:
                return k
        return None

    # the row as it stands (1.5 x row c) may already win again once the ban is lifted; otherwise add the row of a later step's token
    choice = None
    for tok_k in [None] + [t for _, t in ph[1][1:14]]:
        k = first_win(tok_k)
        if k is not None:
            choice = (k, tok_k)
            break
    assert choice is not None, "no step after the first image lets the trigger row win with a margin"
    k, tok_k = choice
    print(f"second image: step {k} of phase 1, {'the row as it stands' if tok_k is None else 'row c + row of token %d' % tok_k}")
    try:
        with torch.no_grad():
            if tok_k is not None:
                W[lay.trigger] = (1.5 * (W[tok_c].float() + W[tok_k].float())).to(W.dtype)
        two = _run(w, ids, 100, max_new_tokens=n_new, max_images=2)
        second = S + j + 1 + lay.block_len + k
        assert two.image_positions == [[S + j, second]] and len(two.images[0]) == 2
        _check_layout(w, two.sequences[0], two.image_positions[0], ids[0], n_new)
        assert two.sequences[0].numel() > second + 1 + lay.block_len            # phase 2: it wrote on after the second <im_end>
        assert torch.equal(two.sequences[0][:second], one.sequences[0][:second])
        assert torch.equal(two.images[0][0], one.images[0][0]) and not torch.equal(two.images[0][1], two.images[0][0])
        capped = _run(w, ids, 100, max_new_tokens=n_new, max_images=1)         # the budget is used up at step k: the id is banned
        assert capped.image_positions == [[S + j]] and len(capped.images[0]) == 1
        assert torch.equal(capped.sequences[0][:second], two.sequences[0][:second])
        assert int(capped.sequences[0][second]) != lay.trigger
    finally:
        with torch.no_grad():
            W[lay.trigger] = saved
