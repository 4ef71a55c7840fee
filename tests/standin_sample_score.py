"""Torch restatement of ops.sample_score (include/mpv.h: mpv_sample_score), test-only, on any device and for bf16 or fp32 logits: the
score_fn of generation.sample_batched_loop when it runs without a GPU, and the reference of the kernel's bookkeeping (count, live and
the entries that stay untouched are compared bitwise; the log-probability itself is compared with an fp64 definition, by both).  It
works in fp32 as the kernel does -- m = max, S = sum exp(x - m), lp = x_t - (m + log S) -- but sums in torch's order, not the
kernel's: its lp is close to the kernel's, not bit-equal."""
import torch


def logprob_row(row: torch.Tensor, t: int) -> torch.Tensor:
    """row [vocab] (any float dtype) -> the fp32 scalar lp of token t as the contract defines it"""
    vocab = row.numel()
    x = row.float()
    if t < 0 or t >= vocab:
        return torch.tensor(float("nan"), dtype=torch.float32, device=row.device)
    if x[t] == float("-inf"):
        return torch.tensor(float("-inf"), dtype=torch.float32, device=row.device)
    m = x.max()
    e = torch.where(x == float("-inf"), torch.zeros_like(x), torch.exp(x - m))
    return x[t] - (m + torch.log(e.sum(dtype=torch.float32)))


def logprob_row_fp64(row: torch.Tensor, t: int) -> float:
    """the definition in fp64: log_softmax in float64 of the same logits; -inf when x_t is -inf (an all -inf row included), NaN when t
    is outside the row"""
    if t < 0 or t >= row.numel():
        return float("nan")
    x = row.double()
    if x[t] == float("-inf"):
        return float("-inf")
    return float(torch.log_softmax(x, dim=0)[t])


def sample_score(logits, st, sc, *, pos, vocab=None, ld=None):
    """ops.sample_score on the tensors of st (generation.SampleState) and sc (generation.SampleScores), row by row; refuses what the
    kernel refuses (AssertionError)"""
    assert logits is not None and st.tokens is not None and st.prompt_len is not None and st.done is not None
    assert sc.live is not None and sc.token_logprob is not None and sc.sum_logprob is not None and sc.count is not None
    vocab = int(vocab) if vocab is not None else logits.shape[-1]
    ld = int(ld) if ld is not None else logits.stride(0)
    assert vocab % 8 == 0 and 8 <= vocab <= 65536 and ld >= vocab and ld % 8 == 0, (vocab, ld)
    assert st.rows >= 1 and 1 <= st.row_len <= 2048 and 0 <= pos < st.row_len, (st.rows, st.row_len, pos)
    assert sc.rows == st.rows and sc.row_len == st.row_len and sc.token_logprob.shape[1] == st.row_len
    for r in range(st.rows):
        if int(st.prompt_len[r]) > pos or int(sc.live[r]) == 0:
            continue
        lp = logprob_row(logits[r, :vocab], int(st.tokens[r, pos]))
        sc.token_logprob[r, pos] = lp
        sc.sum_logprob[r] += lp
        sc.count[r] += 1
        sc.live[r] = 0 if int(st.done[r]) else 1
    return sc
