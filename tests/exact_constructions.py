"""TEST INFRASTRUCTURE: the constructions the bit-exact kernel tests share (tests/test_gpu_kernels_exact.py through the test library,
tests/test_gpu_prefill_exact.py through the engine).  Plain torch on the CPU: activations whose RMS statistics are exact, one-hot
("permutation") weights whose dot products are exact, HF's RoPE tables, the bf16 ulp."""
import torch

BF = torch.bfloat16


def _exact_rows(m, k, g):
    """Rows with mean(x^2) == 1 exactly (k/2 entries of 0.5, 3k/8 of 1, k/8 of 2, random signs and order): the RMS
    statistics are exact in any summation order and x * rsqrt(1 + eps) rounds back to x in bf16."""
    assert k % 8 == 0
    mags = torch.cat([torch.full((k // 2,), 0.5), torch.full((3 * k // 8,), 1.0), torch.full((k // 8,), 2.0)])
    rows = []
    for _ in range(m):
        p = torch.randperm(k, generator=g)
        s = torch.randint(0, 2, (k,), generator=g) * 2 - 1
        rows.append(mags[p] * s)
    return torch.stack(rows).to(BF)


def _gain(k, g):
    vals = torch.tensor([0.5, 0.75, 1.0, 1.25, 1.5, 2.0])
    return vals[torch.randint(0, len(vals), (k,), generator=g)].to(BF)


def _one_hot_rows(n, k, g, signs=True):
    """nn.Linear weight [n][k] whose row j picks input feature sel[j] (times +-1 or +-2): exact dot products."""
    sel = torch.randint(0, k, (n,), generator=g)
    scale = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5])[torch.randint(0, 5 if signs else 1, (n,), generator=g)]
    w = torch.zeros(n, k)
    w[torch.arange(n), sel] = scale
    return w.to(BF), sel, scale


def _rmsnorm_bf16(x, gain, eps):
    x32 = x.float()
    xn = (x32 * torch.rsqrt(x32.pow(2).mean(-1, keepdim=True) + eps)).to(BF)
    return gain * xn


def _rope_table(shape, length, dev):
    """cos / sin exactly as LlamaRotaryEmbedding.forward returns them (fp32 -> bf16), [pos][head_dim]; `shape`: a name of
    synthetic.SHAPES or a LlamaConfig."""
    from layerskip_amd import synthetic
    import transformers
    cfg = synthetic.make_config(shape) if isinstance(shape, str) else shape
    rot = transformers.models.llama.modeling_llama.LlamaRotaryEmbedding(cfg)
    pos = torch.arange(length)[None, :]
    cos, sin = rot(torch.zeros(1, 1, dtype=BF), pos)
    return cos[0].to(dev), sin[0].to(dev)          # [length][hd] bf16


def _bf16_ulp(t):
    return torch.pow(2.0, torch.floor(torch.log2(t.abs().clamp_min(1e-30))) - 7)
