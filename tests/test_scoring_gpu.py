"""`-m gpu`: the scoring kernel (csrc/score.hip) against the float64 restatement (tests/score_ref.py) on the same fp32 logits, the chunked
lm_head + scoring op, and `loglikelihood()` / `choice_logprobs()` against the EXECUTED reference (tests/golden/loglikelihood.pt,
tools/make_golden_score.py: the reference's scoring scripts' arithmetic, one request at a time at batch 1, in fp32 and in bf16)."""
import pytest
import torch

from conftest import check_scalar, check_tensor, rel_l2
from score_ref import score_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

# |kernel - float64| <= ABS + REL * |value| for logprob / lse / cand_logprob.  Derivation: x[t] - max rounds once (<= 6e-8 |x|, |x| <~ 50
# here), the fixed-order tree over <= 40000 positive terms adds <~ log2(V) * 2^-24 ~ 1e-6 relative to the sum, fast exp / log a few ulp;
# the bound is about 5 x that sum.  Measured on the MI355X over every shape below: at most 2.1e-6, 5 % of the bound.
ABS, REL = 2e-5, 2e-6


def _close(name, got, want):
    got, want = got.detach().cpu().double(), want.double()
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got), fin), name
    err = (got[fin] - want[fin]).abs()
    lim = ABS + REL * want[fin].abs()
    worst = float((err / lim).max()) if err.numel() else 0.0
    print(f"{name}: max |err| {float(err.max()) if err.numel() else 0.0:.3e}, {worst:.3f} of the bound")
    assert worst <= 1.0, f"{name}: {worst:.3f} x the bound"
    return worst


def _logits(R, C, V, seed, ties=True):
    """fp32 logits [R, C] as a view with a row pitch that is NOT C, targets with greedy and non-greedy cases, and (from 7 rows on)
    rows built to tie: row 1 two equal maxima with the target on the second, row 2 five equal maxima with the target on the third,
    row 3 the target on the first of three."""
    g = torch.Generator().manual_seed(seed)
    pitch = (C + 3) // 4 * 4 + 8
    buf = torch.randn(R, pitch, generator=g) * 4.0
    x = buf[:, :C]
    tg = torch.randint(0, V, (R,), generator=g)
    am = x[:, :V].argmax(-1)
    tg[::2] = am[::2]
    if ties and R >= 7:
        top = float(x.max()) + 1.0
        x[1, [5, 9]] = top
        tg[1] = 9
        x[2, [3, 40, 77, V - 2, V - 1]] = top
        tg[2] = 77
        x[3, [V - 3, V - 2, V - 1]] = top
        tg[3] = V - 3
        x[4, :V] = 0.0       # a whole row of equal values, one of them -0.0
        x[4, 0] = -0.0
        tg[4] = 6
    return buf.to(DEV)[:, :C], tg.to(DEV)


# ----------------------------------------------------------------------------------------------- 1. kernel vs restatement
@pytest.mark.parametrize("C,limit", [(160, None), (163, None), (5000, None), (32000, None), (32008, 32000), (32008, 32001), (40000, None)],
                         ids=["V160", "V163", "V5000", "V32000", "V32008lim32000", "V32008lim32001", "V40000"])
@pytest.mark.parametrize("R", [1, 7, 300])
def test_score_rows_matches_float64_restatement(C, limit, R):
    """Integer outputs exactly (they depend only on comparisons of the given fp32 values), the floats within ABS / REL.
    Measured on the MI355X: see DESIGN.md §3 (`score_rows_kernel`)."""
    from dreamllm_amd import ops
    V = C if limit is None else limit
    x, tg = _logits(R, C, V, 1000 * R + C)
    assert x.stride(0) != C
    cands = [0, 7, V // 2, V - 1]
    out = ops.score_rows(x, tg, vocab_limit=limit, cand_ids=cands, want_lse=True, want_rank=True)
    ref = score_ref(x, tg, vocab_limit=limit, cand_ids=cands)
    assert int(out.status) == 0
    assert torch.equal(out.argmax.cpu(), ref["argmax"])
    assert torch.equal(out.greedy.cpu(), ref["greedy"])
    assert torch.equal(out.rank.cpu().long(), ref["rank"])
    assert bool(((out.rank == 0) == out.greedy).all())
    for k in ("logprob", "lse", "cand_logprob"):
        _close(f"score_rows[V{V},R{R}].{k}", getattr(out, k), ref[k])
    if R >= 7:
        assert out.greedy[1:5].tolist() == [False, False, True, False] and out.rank[1:5].tolist() == [1, 2, 0, 6]
        assert out.argmax[1:5].tolist() == [5, 3, V - 3, 0]
    assert bool(out.greedy.any())


# ----------------------------------------------------------------------------------------------- 2. special rows
@pytest.mark.parametrize("V", [160, 32000, 40000])
def test_special_rows_are_reported_not_faulted_on(V):
    """target -1, target >= V, a NaN row, a +inf row, a row of -inf: the values and status bits of csrc/score.hip; the rows around them
    are what they are without the special rows.  Every access stays in bounds by construction (the kernel never reads x[t] for a
    target outside [0, V))."""
    from dreamllm_amd import ops
    x, tg = _logits(12, V, V, 5, ties=False)
    x, tg = x.contiguous(), tg.clone()
    clean = ops.score_rows(x, tg, cand_ids=[1, 2], want_lse=True, want_rank=True)
    assert int(clean.status) == 0
    tg[2] = -1
    tg[4] = V + 5
    x[6, V // 3] = float("nan")
    x[8, V - 1] = float("inf")
    x[10, :] = float("-inf")
    tg[10] = -1
    out = ops.score_rows(x, tg, cand_ids=[1, 2], want_lse=True, want_rank=True)
    assert int(out.status) == 3
    normal = [0, 1, 3, 5, 7, 9, 11]
    for k in ("logprob", "lse", "argmax", "greedy", "rank", "cand_logprob"):
        assert torch.equal(getattr(out, k)[normal], getattr(clean, k)[normal]), k
    for r in (2, 4):   # not scored / out of range: the row itself is still summarised
        assert torch.equal(out.lse[r], clean.lse[r]) and torch.equal(out.argmax[r], clean.argmax[r])
        assert torch.equal(out.cand_logprob[r], clean.cand_logprob[r])
        assert not bool(out.greedy[r]) and int(out.rank[r]) == -1
    assert float(out.logprob[2]) == 0.0 and float(out.logprob[4]) == float("-inf")
    for r in (6, 8, 10):
        assert bool(torch.isnan(out.lse[r])) and bool(torch.isnan(out.cand_logprob[r]).all())
        assert int(out.argmax[r]) == 0 and not bool(out.greedy[r]) and int(out.rank[r]) == -1
    assert bool(torch.isnan(out.logprob[6])) and bool(torch.isnan(out.logprob[8])) and float(out.logprob[10]) == 0.0
    only_range = ops.score_rows(x[:6], tg[:6])
    assert int(only_range.status) == 1
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.score_rows(x[:4], tg[:4], status=st)
    assert int(st) == 0
    ops.score_rows(x[6:7], tg[6:7], status=st)
    ops.score_rows(x[:4], tg[:4], status=st)      # the word is only ever OR-ed into
    assert int(st) == 2


def test_score_rows_rejects_bad_arguments():
    from dreamllm_amd import ops
    x, tg = _logits(4, 160, 160, 1)
    with pytest.raises(TypeError):
        ops.score_rows(x.to(BF), tg)
    with pytest.raises(ValueError, match="candidate"):
        ops.score_rows(x, tg, cand_ids=[0, 160])
    with pytest.raises(ValueError, match="candidate"):
        ops.score_rows(x, tg, vocab_limit=100, cand_ids=[100])
    with pytest.raises(ValueError, match="candidate"):
        ops.score_rows(x, tg, cand_ids=list(range(17)))
    with pytest.raises(ValueError):
        ops.score_rows(x, tg[:3])


# ----------------------------------------------------------------------------------------------- 3. determinism, segments
@pytest.mark.parametrize("V", [160, 32000, 40000])
def test_repeat_is_bit_identical_and_segments_add_in_row_order(V):
    from dreamllm_amd import ops
    R = 333
    x, tg = _logits(R, V, V, 11)
    a = ops.score_rows(x, tg, cand_ids=[3, 4, 5], want_lse=True, want_rank=True)
    b = ops.score_rows(x, tg, cand_ids=[3, 4, 5], want_lse=True, want_rank=True)
    for k in ("logprob", "lse", "argmax", "greedy", "rank", "cand_logprob"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    cuts = [0, 1, 1, 5, 70, 71, 200, 333]          # lengths 1, 0, 4, 65, 1, 129, 133
    seg = torch.tensor(cuts, dtype=torch.int64, device=DEV)
    s1 = ops.score_segments(a.logprob, a.greedy, seg)
    s2 = ops.score_segments(a.logprob, a.greedy, torch.tensor(cuts[3:], dtype=torch.int64, device=DEV))   # another N, another grid
    lp, gr = a.logprob.cpu(), a.greedy.cpu()
    want, want_g = [], []
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        acc = torch.zeros((), dtype=torch.float32)
        for r in range(r0, r1):
            acc = acc + lp[r]
        want.append(acc)
        want_g.append(bool(gr[r0:r1].all()))
    assert torch.equal(s1.sum_logprob.cpu(), torch.stack(want)) and s1.all_greedy.cpu().tolist() == want_g
    assert torch.equal(s2.sum_logprob, s1.sum_logprob[3:]) and torch.equal(s2.all_greedy, s1.all_greedy[3:])
    gseg = ops.score_segments(torch.zeros(4, device=DEV), torch.tensor([True, True, False, True], device=DEV),
                              torch.tensor([0, 2, 4], dtype=torch.int64, device=DEV))
    assert gseg.all_greedy.tolist() == [True, False]


# ----------------------------------------------------------------------------------------------- 4. lm_head_score at full width
def test_lm_head_score_full_width_three_chunks(monkeypatch):
    """d = 4096, V = 32008, 3000 scored rows in chunks of 1000 against score_ref applied to ONE `ops.linear_fwd(..., out_dtype=float32)`
    of the same rows (existing code).  The two GEMM calls differ in M and may tile differently, so integers are compared on the rows
    whose top-2 gap in the oracle logits exceeds the largest logit difference between the two GEMM results of this run; at most 2 % of
    the rows may be left out (measured share: DESIGN.md §3)."""
    from dreamllm_amd import ops
    monkeypatch.setattr(ops, "LM_HEAD_CE_CHUNK_ROWS", 1000)
    g = torch.Generator().manual_seed(4)
    T, d, V, R = 3300, 4096, 32008, 3000
    hidden = torch.randn(T, d, generator=g).to(BF).to(DEV)
    w = (torch.randn(V, d, generator=g) * 0.02).to(BF).to(DEV)
    rows = torch.randperm(T, generator=g)[:R].sort().values.to(DEV)
    tg = torch.randint(0, V, (R,), generator=g).to(DEV)
    cands = [319, 350, 315, 360]
    seg = torch.tensor([0, 10, 1500, 3000], dtype=torch.int64, device=DEV)
    with torch.no_grad():
        oracle = ops.linear_fwd(ops.gather_rows(hidden, rows), ops._pad_vocab(w), out_dtype=torch.float32)[:, :V]
        tg[::3] = oracle.argmax(-1)[::3]
        out = ops.lm_head_score(hidden, w, rows, tg, cand_ids=cands, seg_start=seg, want_lse=True, want_rank=True)
        h = ops.gather_rows(hidden, rows)
        gemm_diff = max(float((ops.linear_fwd(h[r0:r0 + 1000], ops._pad_vocab(w), out_dtype=torch.float32)[:, :V] - oracle[r0:r0 + 1000]).abs().max())
                        for r0 in range(0, R, 1000))
    assert int(out.status) == 0
    oc = oracle.cpu()
    ref = {}
    for r0 in range(0, R, 500):
        part = score_ref(oc[r0:r0 + 500], tg[r0:r0 + 500], cand_ids=cands)
        for k, v in part.items():
            ref.setdefault(k, []).append(v)
    ref = {k: torch.cat(v) for k, v in ref.items()}
    top2 = oc.topk(2, dim=-1).values
    gap = top2[:, 0] - top2[:, 1]
    keep = gap > gemm_diff
    left_out = 1.0 - float(keep.float().mean())
    print(f"lm_head_score: largest logit difference between the two GEMM calls {gemm_diff:.3e}; {left_out:.2%} of {R} rows left out of the "
          f"integer comparison (top-2 gap median {float(gap.median()):.3e})")
    assert left_out <= 0.02
    for k in ("logprob", "lse", "cand_logprob"):
        _close(f"lm_head_score.{k}", getattr(out, k), ref[k])
    assert torch.equal(out.argmax.cpu()[keep], ref["argmax"][keep])
    assert torch.equal(out.greedy.cpu()[keep], ref["greedy"][keep])
    tkeep = keep & ((oc.gather(1, tg.cpu()[:, None])[:, 0][:, None] - oc).abs() > gemm_diff).sum(-1).ge(V - 1)   # no other logit within reach of the target's
    assert torch.equal(out.rank.cpu().long()[tkeep], ref["rank"][tkeep]) and float(tkeep.float().mean()) > 0.5
    want_sum = torch.stack([out.logprob[a:b].cpu().double().sum() for a, b in [(0, 10), (10, 1500), (1500, 3000)]])
    assert float((out.sum_logprob.cpu().double() - want_sum).abs().max()) <= 1e-3 * 1.0 + 2e-6 * float(want_sum.abs().max())
    assert out.all_greedy.tolist() == [bool(out.greedy[a:b].all()) for a, b in [(0, 10), (10, 1500), (1500, 3000)]]


# ----------------------------------------------------------------------------------------------- 5. against the executed reference
def _build(case):
    from dreamllm_amd.configuration_dreamllm import DreamLLMConfig
    from dreamllm_amd.modeling_dreamllm import DreamLLMForCausalMLM
    from oracle import llm_ref
    from oracle.make_golden import special_tokens2ids_dict
    lm = DreamLLMForCausalMLM(DreamLLMConfig(**case["cfg"], special_tokens2ids_dict=special_tokens2ids_dict()))
    res = lm.load_state_dict(llm_ref.random_state_dict(case["cfg"], case["seed"], **case["sd_kwargs"]), strict=False)
    assert not res.unexpected_keys and all("inv_freq" in k for k in res.missing_keys)
    return lm.to(DEV, BF).eval()


def _limit(case):
    return None if case["vocab_limit"] == case["cfg"]["vocab_size"] else case["vocab_limit"]


def _check_against_fixture(tag, f, c, out):
    """Token log-probs and sums under the 1.15 x err_ref + 5e-4 contract with the bf16 reference as yard-stick; is_greedy and the chosen
    ending of each item only where the reference is decidable (tools/make_golden_score.py), with the caps asserted."""
    ref, refb = torch.cat(c["token_logprobs"]), torch.cat(c["token_logprobs_bf16"])
    ours = torch.cat([t.float().cpu() for t in out.token_logprobs])
    assert [t.numel() for t in out.token_logprobs] == c["num_tokens"].tolist()
    check_tensor(f"{tag}.token_logprobs", ours, ref, rel_l2(refb, ref))
    assert out.num_tokens.cpu().tolist() == c["num_tokens"].tolist()
    assert out.sum_logprob.dtype == torch.float32 and out.num_tokens.dtype == torch.int64 and out.is_greedy.dtype == torch.bool
    for i in range(len(c["requests"])):
        check_scalar(f"{tag}.sum_logprob[{i}]", out.sum_logprob[i], c["sum_logprob"][i],
                     ref_bf16_abs_err=float((c["sum_logprob_bf16"][i] - c["sum_logprob"][i]).abs()))
    # is_greedy: a request with a decidable non-greedy token must come out False, one whose tokens are all decidable and greedy True;
    # a request that hinges on an undecidable token is left out
    total = left = compared = 0
    for i in range(len(c["requests"])):
        dec = c["top2_gap"][i] >= f["gap_factor"] * c["logit_err_bf16"][i]
        total += dec.numel()
        left += int((~dec).sum())
        if bool((dec & ~c["greedy"][i]).any()):
            assert not bool(out.is_greedy[i]), (tag, i)
            compared += 1
        elif bool(dec.all()):
            assert bool(out.is_greedy[i]) == bool(c["greedy"][i].all()), (tag, i)
            compared += 1
    assert left <= f["max_tokens_out"] * total and compared >= 1, (left, total, compared)
    items_out = 0
    for it in sorted(set(c["item_of"])):
        idx = [i for i, v in enumerate(c["item_of"]) if v == it]
        s, sb = c["sum_logprob"][idx], c["sum_logprob_bf16"][idx]
        top = s.topk(2).values
        if float(top[0] - top[1]) >= f["gap_factor"] * float((sb - s).abs().max()):
            assert int(out.sum_logprob[idx].argmax()) == int(s.argmax()), (tag, it)
        else:
            items_out += 1
    assert items_out <= f["max_items_out"]
    print(f"{tag}: {left}/{total} tokens and {items_out} items undecidable; {compared} requests' is_greedy compared")


@pytest.mark.parametrize("name", ["tiny", "big_limit", "big_full"])
def test_loglikelihood_matches_executed_reference(golden, name):
    f = golden("loglikelihood.pt")
    c = f[name]
    lm = _build(c)
    out = lm.loglikelihood(c["requests"], vocab_limit=_limit(c), return_token_logprobs=True)
    _check_against_fixture(f"loglikelihood[{name}]", f, c, out)
    plain = lm.loglikelihood(c["requests"], vocab_limit=_limit(c))
    assert plain.token_logprobs is None and torch.equal(plain.sum_logprob, out.sum_logprob)
    if name == "big_limit":   # the limit decides: without it the boosted added tokens take the arg-max of rows the limited call calls greedy
        full = lm.loglikelihood(c["requests"])
        assert bool((full.sum_logprob < out.sum_logprob).all()) and bool((full.is_greedy <= out.is_greedy).all())
        with pytest.raises(ValueError, match="request 0"):
            lm.loglikelihood([([1, 32001], [5])], vocab_limit=32000)


@pytest.mark.parametrize("name", ["tiny", "big_limit", "big_full"])
@pytest.mark.parametrize("side", ["left", "right"])
def test_choice_logprobs_matches_executed_reference(golden, name, side):
    f = golden("loglikelihood.pt")
    c = f[name]
    lr, s = c["last_row"], c["last_row"][side]
    lm = _build(c)
    lp, am = lm.choice_logprobs(s["input_ids"].to(DEV), lr["candidate_ids"], attention_mask=s["attention_mask"].to(DEV),
                                vocab_limit=_limit(c))
    assert lp.shape == (4, 4) and lp.dtype == torch.float32 and am.dtype == torch.int64
    check_tensor(f"choice_logprobs[{name},{side}]", lp, s["cand_logprob"], rel_l2(s["cand_logprob_bf16"], s["cand_logprob"]))
    dec = s["top2_gap"] >= f["gap_factor"] * s["logit_err_bf16"]
    assert int((~dec).sum()) <= f["max_items_out"]
    assert torch.equal(am.cpu()[dec], s["argmax"][dec])
    if side == "right":   # the same prompts one by one, unpadded: the last row is simply S - 1
        single = [lm.choice_logprobs(torch.tensor([p], device=DEV), torch.tensor(lr["candidate_ids"]), vocab_limit=_limit(c))[0][0]
                  for p in lr["prompts"]]
        check_tensor(f"choice_logprobs[{name},one by one]", torch.stack(single), s["cand_logprob"],
                     rel_l2(s["cand_logprob_bf16"], s["cand_logprob"]))
    with pytest.raises(ValueError):
        lm.choice_logprobs(s["input_ids"].to(DEV), list(range(17)))


# ----------------------------------------------------------------------------------------------- 6. batching
def test_batching_and_order_do_not_matter_beyond_rounding(golden):
    f = golden("loglikelihood.pt")
    c = f["tiny"]
    lm = _build(c)
    ref, refb = torch.cat(c["token_logprobs"]), torch.cat(c["token_logprobs_bf16"])
    yard = rel_l2(refb, ref)
    cat = lambda o: torch.cat([t.float().cpu() for t in o.token_logprobs])  # noqa: E731
    one = lm.loglikelihood(c["requests"], max_batch_rows=1, return_token_logprobs=True)
    many = lm.loglikelihood(c["requests"], max_batch_rows=64, return_token_logprobs=True)
    tight = lm.loglikelihood(c["requests"], max_batch_tokens=40, return_token_logprobs=True)
    perm = torch.randperm(len(c["requests"]), generator=torch.Generator().manual_seed(1)).tolist()
    shuf = lm.loglikelihood([c["requests"][i] for i in perm], return_token_logprobs=True)
    inv = [perm.index(i) for i in range(len(perm))]
    shuf_tokens = torch.cat([shuf.token_logprobs[j].float().cpu() for j in inv])
    _check_against_fixture("loglikelihood[tiny,rows=1]", f, c, one)
    check_tensor("loglikelihood rows=64 vs rows=1", cat(many), cat(one), yard)
    check_tensor("loglikelihood rows=1 vs rows=64", cat(one), cat(many), yard)
    check_tensor("loglikelihood tokens<=40 vs rows=64", cat(tight), cat(many), yard)
    check_tensor("loglikelihood shuffled vs in order", shuf_tokens, cat(many), yard)
    for o in (one, many, tight):
        assert o.num_tokens.cpu().tolist() == c["num_tokens"].tolist()
    assert shuf.num_tokens.cpu().tolist() == [int(c["num_tokens"][i]) for i in perm]
    for i in range(len(perm)):
        check_scalar(f"shuffled.sum_logprob[{i}]", shuf.sum_logprob[inv[i]], many.sum_logprob[i],
                     ref_bf16_abs_err=float((c["sum_logprob_bf16"][i] - c["sum_logprob"][i]).abs()))


def test_loglikelihood_reports_non_finite_logits(golden):
    c = golden("loglikelihood.pt")["tiny"]
    lm = _build(c)
    with torch.no_grad():
        lm.lm_head.weight[3, 0] = float("nan")
    with pytest.raises(FloatingPointError, match="request 0"):
        lm.loglikelihood(c["requests"][:3])


# ----------------------------------------------------------------------------------------------- 7. perplexity of a document
def test_rolling_perplexity_matches_the_fused_ce_loss(monkeypatch):
    """One 3000-token document at 2 layers x 7B width: loglikelihood([(ids[:1], ids[1:])]) against the project's own fused lm_head + CE
    loss x (S - 1).  2999 scored rows in chunks of 1024: the large-R, multi-chunk case."""
    from dreamllm_amd import ops
    from dreamllm_amd.factory import VICUNA_7B, build_dreamllm
    monkeypatch.setattr(ops, "LM_HEAD_CE_CHUNK_ROWS", 1024)
    S = 3000
    lm = build_dreamllm(dict(VICUNA_7B, num_hidden_layers=2, max_position_embeddings=4096), device=DEV, with_clip=False, with_sd=False).eval()
    ids = torch.randint(3, 32000, (S,), generator=torch.Generator().manual_seed(8))
    out = lm.loglikelihood([(ids[:1], ids[1:])])
    with torch.no_grad():
        loss = lm(input_ids=ids[None].to(DEV), labels=ids[None].to(DEV), return_dict=True).loss
    assert int(out.num_tokens[0]) == S - 1
    check_scalar("rolling perplexity: -sum_logprob vs loss x (S - 1)", -float(out.sum_logprob[0]), float(loss) * (S - 1), rtol=1e-3)
    print(f"perplexity {float(torch.exp(-out.sum_logprob[0] / (S - 1))):.1f} (loss {float(loss):.4f})")
