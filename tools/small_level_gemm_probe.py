"""The Linear products of levels 3-5 (12,496 x 128, 3,124 x 256, 780 x 512 rows) through csrc/rowlin2_impl.h.

Without arguments: each plain product against the library GEMM of the same shape -- how far the streaming skinny-GEMM kernels (built for
10^5 rows x 32-64 channels) are from a tiled GEMM where the rows are few.

With --baseline-lib <libpdfops.so of the parent commit>: the q / k / v product, the three-input input gradient with BatchNorm sums, the
c x c products with statistics and the accumulating transposed product, this build against the parent's library alternating in one
process.  One call between two device events per sample (a filler kernel in front keeps the device busy while the host enqueues, so the
interval holds no host time), median / p10 / p90 of --rounds samples after warm-up, for the parent, for this build with PDFOPS_RL_FORM =
slab, group and auto.  A shape has earned the group form when its group median is below the parent's by more than the parent's p90 - p10."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pointcloudpdf_amd import _native

be = _native.hip_backend()
torch.backends.cuda.matmul.allow_tf32 = False


def t(fn, it=50):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it * 1e3


def library_table():
    for n, k, o in [(780, 512, 512), (3124, 256, 256), (12496, 128, 128), (49984, 64, 64), (200000, 32, 32), (780, 512, 1536), (3124, 256, 768)]:
        x = torch.randn(n, k, device="cuda"); w = torch.randn(o, k, device="cuda") / k ** 0.5; g = torch.randn(n, o, device="cuda")
        gf = 2.0 * n * k * o / 1e9
        a = t(lambda: be.rowlin(x, w, None)); b = t(lambda: torch.nn.functional.linear(x, w))
        c = t(lambda: be.rowlin(g, w, transpose_w=True)); d = t(lambda: g @ w)
        e = t(lambda: be.rowlin_wgrad(g, x, None, False, False)); f = t(lambda: g.t() @ x)
        print(f"n={n:6d} k={k:4d} o={o:4d} ({gf:5.2f} GFLOP): fwd {a:6.1f} us (lib {b:6.1f})  dgrad {c:6.1f} (lib {d:6.1f})  wgrad {e:6.1f} (lib {f:6.1f})   fwd {gf / a * 1e3:5.1f} TFLOP/s", flush=True)


def launches(n, c):
    """name -> callable(backend) for the launches of one level (n rows, c channels)"""
    g = torch.Generator(device="cuda").manual_seed(n + c)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x, go, y0 = r(n, c), r(n, c), r(n, c)
    ws = [r(c, c) / c ** 0.5 for _ in range(3)]
    bs = [r(c) for _ in range(3)]
    gs = [r(n, c) for _ in range(3)]
    sc = torch.rand(c, device="cuda", generator=g) + 0.5
    coef = torch.cat([sc, r(c) * 0.3, x.mean(0), (x.var(0, unbiased=False) + 1e-5).rsqrt()])
    out = {
        "qkv (pre)": lambda b: b.rowlin_multi([x], ws, bs, coef=coef, relu=True, nout=3),
        "c x c + stats (pre)": lambda b: b.rowlin(x, ws[0], bs[0], coef=coef, relu=True, stats=True),
        "c x c + stats": lambda b: b.rowlin(x, ws[0], bs[0], stats=True),
        "c x c transposed, accumulate": lambda b: b.rowlin(go, ws[0], transpose_w=True, out=y0, accumulate=True),
    }
    if c <= 256:   # (three inputs at 512: three accumulating launches of the line above)
        out["dgrad, 3 inputs + BN sums"] = lambda b: b.rowlin_dgrad_bn_backward(gs, ws, x, coef, training=True, relu=True)
    return out


def compare(baseline_lib, rounds, out_path):
    parent = _native.HipBackend(_native.load_library(os.path.abspath(baseline_lib)))
    filler = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    sides = [("parent", parent, None), ("slab", be, "slab"), ("group", be, "group"), ("auto", be, None)]

    def sample(fn, b, form):
        if form is None:
            os.environ.pop("PDFOPS_RL_FORM", None)
        else:
            os.environ["PDFOPS_RL_FORM"] = form
        filler.fill_(1)
        e0.record(); fn(b); e1.record()
        e1.synchronize()
        os.environ.pop("PDFOPS_RL_FORM", None)
        return e0.elapsed_time(e1) * 1e3

    lines = [f"# us per call: median (p10 .. p90) of {rounds} alternating samples; 'earned': group median < parent median - (parent p90 - p10)",
             f"{'shape':>12}  {'launch':<30}" + "".join(f"{s[0]:>24}" for s in sides) + "  earned"]
    print("\n".join(lines), flush=True)
    for n, c in [(12496, 128), (3124, 256), (780, 512)]:
        for name, fn in launches(n, c).items():
            for _ in range(5):
                for _, b, form in sides: sample(fn, b, form)
            v = {s[0]: [] for s in sides}
            for _ in range(rounds):
                for s, b, form in sides: v[s].append(sample(fn, b, form))
            q = {s: np.percentile(np.array(a), [50, 10, 90]) for s, a in v.items()}
            earned = q["group"][0] < q["parent"][0] - (q["parent"][2] - q["parent"][1])
            line = f"{n:>6} x {c:<4} {name:<30}" + "".join(f"{q[s[0]][0]:>9.1f} ({q[s[0]][1]:5.1f} ..{q[s[0]][2]:5.1f})" for s in sides) + f"  {'yes' if earned else 'no'}"
            print(line, flush=True)
            lines.append(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", help="libpdfops.so of the parent commit: compare this build's launches against it")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--out", help="write the comparison table here")
    args = ap.parse_args()
    if args.baseline_lib:
        compare(args.baseline_lib, max(args.rounds, 30), args.out)
    else:
        library_table()
