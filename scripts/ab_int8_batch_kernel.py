"""A/B driver for the build-time choices of the int8 batch pass (csrc/knn_mfma_i8.hip: DEWI_I8_NT, DEWI_I8_ITEM_STEPS).

One process per build: the library is chosen by DEWI_HIP_LIB, the line label by --label.  Build a variant next to the
default library with, from the package's csrc directory,

    make OBJDIR=../build/nt1 OUTDIR=../lib_nt1 \\
         CXXFLAGS="-O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function --offload-arch=gfx950 -DDEWI_I8_NT=1"

and run

    DEWI_HIP_LIB=<package>/lib_nt1/libdewi_hip.so python scripts/ab_int8_batch_kernel.py --label "DEWI_I8_NT=1 DEWI_I8_ITEM_STEPS=8"

Per dim (768, 256, 1536) and cut (20, 200): 1 048 576 rows of random codes made on the device, 32 random queries, the C entry
point dewi_knn_candidates_i8_batch alone.  `call`: events around 200 back-to-back calls, median (min-max) of 3 rounds after 5
warm-up calls.  `pass kernel`: the library's own bracket around the full-pass kernel (dewi_timing_enable), mean of 50 calls,
and its algorithmic bytes n (dim + 4) + 32 dim over that time.
"""
import argparse
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "dewi-design-for-an-entropy-weighted-index-for-text-image-corpora_amd"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this build")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dims", default="768,256,1536")
    a = ap.parse_args()

    import torch
    from dewi import _engine as eng
    from dewi import _native as nat

    lib = nat.load_library()
    n, b = a.n, 32
    for dim in (int(x) for x in a.dims.split(",")):
        g = torch.Generator(device="cuda").manual_seed(1)
        codes = torch.randint(-127, 128, (n, dim), dtype=torch.int8, device="cuda", generator=g)
        scales = torch.rand(n, device="cuda", generator=g) * 0.01 + 0.001
        Q = torch.randn(b, dim, device="cuda", generator=g)
        pay = torch.rand(n, device="cuda")
        for c in (20, 200):
            need = lib.dewi_knn_i8_batch_workspace_bytes(n, dim, b, c)
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            out = torch.empty((b, c, 4), dtype=torch.int32, device="cuda")

            def call():
                nat.check(lib.dewi_knn_candidates_i8_batch(nat.ptr(codes), nat.ptr(scales), n, dim, nat.ptr(Q), b, nat.ptr(pay),
                                                           nat.ptr(pay), c, 0, nat.ptr(out), nat.ptr(ws), need, nat.stream_ptr()))

            for _ in range(5):
                call()
            torch.cuda.synchronize()
            whole = []
            for _ in range(3):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(200):
                    call()
                t1.record()
                torch.cuda.synchronize()
                whole.append(t0.elapsed_time(t1) / 200)
            eng.timing(1)
            for _ in range(50):
                call()
            torch.cuda.synchronize()
            ms, _ = eng.timing_read()
            eng.timing(0)
            rate = (n * (dim + 4) + 32 * dim) / ms / 1e9
            print(f"{a.label:<40} dim {dim} c {c}: call {statistics.median(whole):.4f} ms ({min(whole):.4f}-{max(whole):.4f}), "
                  f"pass kernel {ms:.4f} ms = {rate:.3f} TB/s", flush=True)
        del codes


if __name__ == "__main__":
    main()
