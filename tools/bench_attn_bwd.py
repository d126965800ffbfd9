"""Times the stand-alone attention operators at the head shapes of the training steps (Visformer stages 2 and 3 of an 800-image step, DeiT-S of a
256-image step):  python tools/bench_attn_bwd.py [f32|bf16|fwd] [variant .so]
f32 / bf16: fsvit_attention_backward in that storage type; fwd: fsvit_attention (ops.attention) in both."""
import sys
import torch
import os
sys.path.insert(0, '.')
from fewshot_vit_amd import _lib            # noqa: E402
if len(sys.argv) > 2:                       # a variant library
    _lib.LIB_PATH = os.path.abspath(sys.argv[2])
from fewshot_vit_amd.engine import ops      # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else 'f32'
if mode not in ('f32', 'bf16', 'fwd'):
    sys.exit(f'mode: f32, bf16 or fwd, got {mode!r}')
# (S, hd, hdp, heads, B); DeiT-S: attention_bwd_mfma_kernel<14, 4, 4> / attention_bwd_f32mfma_long_kernel<13, 4, 7>
SHAPES = ((100, 42, 48, 6, 800), (25, 85, 96, 6, 800), (197, 64, 64, 6, 256))


def timed(call):
    for _ in range(3):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 10


for dt in ((torch.float32, torch.bfloat16) if mode == 'fwd' else (torch.float32 if mode == 'f32' else torch.bfloat16,)):
    for S, hd, hdp, heads, B in SHAPES:
        if mode != 'fwd' and dt == torch.bfloat16 and hdp % 32:
            hdp = (hdp + 31) // 32 * 32
        qkv = torch.zeros(B, S, 3, heads, hdp)
        qkv[..., :hd] = torch.randn(B, S, 3, heads, hd)
        dctx = torch.zeros(B, S, heads, hdp)
        dctx[..., :hd] = torch.randn(B, S, heads, hd)
        q, d = qkv.to(dt).cuda().view(B * S, -1), dctx.to(dt).cuda().view(B * S, -1)
        if mode == 'fwd':
            ms = timed(lambda: ops.attention(q, B, S, heads, hdp, hd ** -0.5))
            fl = B * heads * 2 * 2.0 * S * S * hd
        else:
            ms = timed(lambda: ops.attention_backward(q, d, B, S, heads, hd, hdp, hd ** -0.5))
            fl = B * heads * 5 * 2.0 * S * S * hd
        print(f'attention {"forward" if mode == "fwd" else "backward"} {dt} B={B} S={S} hd={hd}: {ms * 1e3:.1f} us, {fl / ms / 1e9:.1f} TFLOP/s')
