"""GPU (-m gpu): a launch census of the encoder graph.

Every encoder contraction chooses its kernel by itself (the plane kernels, or the fp32-storage fall-back kernels when the
load-time slack check or the test hook force_fallback flags it, or when gemm_variant / attn_variant force them), and a
tensor's format follows its one consumer.  The kernel-class timers (kernel_timers = 1, wt_last_kernel_stats) count the
launches of a pass per class; the expected counts come from the small model of that hand-over rule below, so a launch
that goes missing, doubles or changes class in any mode of the graph shows here.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def expected_census(L, mask=0, attn_variant=4, gemm_variant=-1, bf16=False, absorbed=False):
    """Launches per kernel-class name of one encoder pass.  Contraction i of force_fallback, in launch order: conv1 0,
    conv2 1, layer l: qkv 2 + 5 l, attention 3 + 5 l, out 4 + 5 l, fc1 5 + 5 l, fc2 6 + 5 l, cross-KV 2 + 5 L."""
    n_gemm = 2 + 4 * L + (0 if absorbed else 1)
    if bf16:  # every contraction in the default class, under the bf16 names; nothing to hand over
        return {"gemm_bf16_planes": n_gemm, "encoder_attention_bf16": L, "gemm_split16_tile": 0,
                "encoder_attention_split": 0, "f32_to_planes": 0, "mel_transpose": 1}

    def planes(i):
        return gemm_variant < 0 and not (mask >> i) & 1

    gemms = [0, 1] + [2 + 5 * l + j for l in range(L) for j in (0, 2, 3, 4)] + ([] if absorbed else [2 + 5 * L])
    on_planes = sum(planes(i) for i in gemms)
    convert = int(not planes(0) and planes(1))
    attn_planes = 0
    for l in range(L):
        qkv, att, out, fc1, fc2 = (2 + 5 * l + j for j in range(5))
        ap = gemm_variant < 0 and attn_variant == 4 and not (mask >> att) & 1 and planes(out)
        attn_planes += ap
        convert += (not planes(qkv) and ap) + (not ap and planes(out)) + (not planes(fc1) and planes(fc2))
    census = {"gemm_planes": on_planes, "encoder_attention_planes": attn_planes, "f32_to_planes": convert, "mel_transpose": 1}
    alt_gemm = "gemm_f32_tile" if gemm_variant == 0 else "gemm_split16_tile"
    alt_attn = "encoder_attention_f32" if attn_variant == 0 else "encoder_attention_split"
    census[alt_gemm] = len(gemms) - on_planes
    census[alt_attn] = L - attn_planes
    return census


def test_census_model_on_known_passes():
    """The model itself, on passes whose counts DESIGN.md and test_gpu_boundary.py state (tiny, L = 4)."""
    c = expected_census(4)
    assert (c["gemm_planes"], c["encoder_attention_planes"], c["f32_to_planes"]) == (19, 4, 0)
    assert expected_census(4, absorbed=True)["gemm_planes"] == 18
    c = expected_census(4, (1 << 3) | (1 << 4))  # layer 0's attention and out-projection: fall-back feeds fall-back
    assert (c["gemm_planes"], c["gemm_split16_tile"], c["encoder_attention_planes"], c["f32_to_planes"]) == (18, 1, 3, 0)
    c = expected_census(4, 1 << 4, attn_variant=1)
    assert (c["encoder_attention_split"], c["f32_to_planes"], c["gemm_planes"]) == (4, 3, 18)
    assert expected_census(4, (1 << 5) | (1 << 6))["f32_to_planes"] == 0
    assert expected_census(4, 1 << 5)["f32_to_planes"] == 1
    c = expected_census(4, (1 << 23) - 1)
    assert (c["gemm_planes"], c["gemm_split16_tile"], c["encoder_attention_split"], c["f32_to_planes"]) == (0, 19, 4, 0)


class _Census:
    """One engine per model size for all cases: a case sets every option it depends on and puts the defaults back."""

    def __init__(self, pkg, assets, arch):
        prefix, vocab = assets(arch)
        self.e = e = pkg.Engine(prefix, vocab, True)
        self.L = e.dims.n_audio_layer
        e.set_option("stop_at_eot", 0)
        e.set_option("max_tokens", 4)  # the smallest the option takes
        e.set_option("kernel_timers", 1)
        if arch == "micro":
            e.set_prompt([3, 5, 7, 11])  # the micro vocabulary has no special ids
        self.mel1 = np.random.default_rng(21).uniform(-1.0, 1.5, size=(1,) + e.mel_shape).astype(np.float32)

    def run(self, mask=0, attn_variant=4, gemm_variant=-1, bf16=0, clips=1):
        e = self.e
        e.set_option("force_fallback", mask)
        e.set_option("attn_variant", attn_variant)
        e.set_option("gemm_variant", gemm_variant)
        e.set_option("bf16", bf16)
        try:
            assert e.get_option("f16_fallbacks") == bin(mask).count("1")  # the precondition of the model's `mask` input
            mel = self.mel1 if clips == 1 else np.zeros((clips,) + e.mel_shape, np.float32)
            e.encdec_tokens_batch(mel)
            ks = {k: v["launches"] for k, v in e.kernel_stats().items()}
        finally:
            e.set_option("bf16", 0)
            e.set_option("gemm_variant", -1)
            e.set_option("attn_variant", 4)
            e.set_option("force_fallback", 0)
        # the absorbed cross-attention (no cross-KV GEMM): synchronous calls from 32 clips on, when its operand is on planes
        absorbed = clips >= 32 and (bool(bf16) or (gemm_variant < 0 and not (mask >> (2 + 5 * self.L)) & 1))
        want = expected_census(self.L, mask, attn_variant, gemm_variant, bool(bf16), absorbed)
        got = {k: ks.get(k, 0) for k in want}
        print("census", dict(mask=hex(mask), av=attn_variant, gv=gemm_variant, bf16=bf16, clips=clips), ks)
        assert got == want, (ks, want)
        return ks["layernorm_rows"]


@pytest.fixture(scope="module")
def tiny(pkg, assets):
    c = _Census(pkg, assets, "tiny")
    yield c
    c.e.close()


TINY_CASES = ([dict(mask=0)] + [dict(mask=1 << i) for i in range(23)] +
              [dict(mask=(1 << 2) | (1 << 4)), dict(mask=(1 << 5) | (1 << 6)), dict(mask=(1 << 23) - 1),
               dict(attn_variant=1), dict(attn_variant=0), dict(gemm_variant=0), dict(gemm_variant=13),
               dict(bf16=1), dict(clips=32), dict(clips=32, bf16=1)])


@pytest.mark.parametrize("case", TINY_CASES, ids=lambda c: "-".join(f"{k}{v:x}" for k, v in c.items()))
def test_tiny_launch_census(tiny, case):
    """Which GEMM tiles fuse the LayerNorm that follows them is the kernels' business (384-column tiles, d = 384), so the
    LayerNorm launches are only bounded: at most one per LayerNorm of the graph, and in bf16 storage mode at least the
    ln_post record, which that mode keeps whether or not the LayerNorm was fused."""
    ln = tiny.run(**case)
    assert ln <= 2 * tiny.L + 1
    if case.get("bf16"):
        assert ln >= 1


@pytest.mark.parametrize("bf16", [0, 1])
def test_micro_launch_census_counts_every_layernorm(pkg, assets, bf16):
    """d = 128, where the LayerNorm count is exact.  The plane GEMM fuses a LayerNorm only in its 384-column tiles, so
    every LayerNorm of the graph is a launch of its own: 2 L + 1.  The bf16 GEMM has a whole-row tile for d = 128 too
    (k_gemm_bf16.hip), so there every one is fused, and what is left is the ln_post record that mode always keeps: 1."""
    c = _Census(pkg, assets, "micro")
    try:
        assert c.run(bf16=bf16) == (1 if bf16 else 2 * c.L + 1)
    finally:
        c.e.close()
