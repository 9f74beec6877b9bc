"""Same-box A/B of gp_gemm_ex between library builds: every library given is loaded into this one
process (ctypes, RTLD_LOCAL: each keeps its own code objects) and multiplies the same seeded
operands.  The GEMM is deterministic (split-K slices are reduced in a fixed order), so every
output must be byte-equal to the first library's; the four ensemble-streaming products of
randomized_svd are also timed with HIP events, the libraries alternating window by window.

    python tools/ab_gemm_libs.py [--small-only] parent.so new.so [...]

Shapes: the fit's 512 runs x 1,347,945 locations at r = 25, once as a float32 ensemble (the 8-B
tsk form) and once as an fp64 ensemble at the padded row stride of emulator.standardize_y (the
16-B form); and the tall-skinny edge shapes of tests/test_gpu_fitside.py.  A product's speed
holds if a library's median window is not above the first library's slowest window.
Exit status 1 if any byte differs."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gladsgp_amd.blas import CM  # noqa: E402  (torch's HIP runtime first)

F64 = torch.float64
WARM, WINDOWS, CALLS = 3, 8, 5          # per library and product: calls, timed windows, calls each
small_only = "--small-only" in sys.argv
libs = []
for path in [a for a in sys.argv[1:] if not a.startswith("--")]:
    h = ctypes.CDLL(os.path.abspath(path))
    h.gp_dgemm_ws_bytes.argtypes = [ctypes.c_int] * 3
    h.gp_dgemm_ws_bytes.restype = ctypes.c_longlong
    h.gp_gemm_ex.argtypes = ([ctypes.c_int] * 5 + [ctypes.c_double, ctypes.c_void_p, ctypes.c_int,
                                                   ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                   ctypes.c_int, ctypes.c_double, ctypes.c_void_p,
                                                   ctypes.c_int, ctypes.c_void_p,
                                                   ctypes.c_longlong, ctypes.c_void_p])
    libs.append((os.path.basename(path), h))
assert len(libs) >= 2, __doc__
dev = torch.device("cuda:0")
st = torch.cuda.current_stream(dev).cuda_stream
ws = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
bad = 0


def gemm(h, ta, tb, A, B, C, alpha=1.0, beta=0.0):
    m, k = (A.cols, A.rows) if ta else (A.rows, A.cols)
    n = B.rows if tb else B.cols
    need = h.gp_dgemm_ws_bytes(m, n, k)
    assert need <= ws.numel(), (m, n, k, need)
    rc = h.gp_gemm_ex(int(ta), int(tb), m, n, k, alpha, A.ptr(), int(A.f32), A.ld, B.ptr(),
                      int(B.f32), B.ld, beta, C.ptr(), C.ld, ws.data_ptr(), need, st)
    assert rc == 0, rc
    return C


def same(tag, outs):
    """Every library's output against the first's, byte for byte."""
    global bad
    torch.cuda.synchronize()
    for (name, _), o in zip(libs[1:], outs[1:]):
        a, b = outs[0].t.view(torch.int64), o.t.view(torch.int64)
        ndiff = int((a != b).sum())
        bad += ndiff > 0
        print(f"bits {tag:44s} {name:24s} {'equal' if ndiff == 0 else 'DIFFERENT'} "
              f"({ndiff} of {a.numel()} differ)", flush=True)


def cm(M, dt):
    """A numpy (rows x cols) matrix as a tight column-major operand of dtype dt."""
    return CM(torch.as_tensor(M.T.copy(), device=dev).to(dt), M.shape[0], M.shape[1], M.shape[0])


def padded(X):
    """A C-order ensemble at standardize_y's row stride, the padding NaN; as (locations x runs)."""
    runs, big = X.shape
    ld = (big + 15) // 16 * 16
    pad = torch.full((runs, ld), float("nan"), dtype=F64, device=dev)
    pad[:, :big] = torch.as_tensor(X, device=dev)
    return CM(pad, big, runs, ld)


# ---- the tall-skinny edge shapes of the GPU tests ---------------------------------------------
for m, n, k in ((256, 25, 66000), (65, 32, 65537), (1, 1, 65536)):
    for ta, tb in ((0, 0), (0, 1), (1, 0), (1, 1)):
        rng = np.random.default_rng(7 * m + n + k + ta * 2 + tb)
        A = rng.standard_normal((k, m) if ta else (m, k)).astype(np.float32)
        B = rng.standard_normal((n, k) if tb else (k, n)).astype(np.float32)
        C0 = rng.standard_normal((m, n))
        for fa, fb in ((0, 0), (1, 0), (0, 1), (1, 1)):
            Ac, Bc = cm(A, torch.float32 if fa else F64), cm(B, torch.float32 if fb else F64)
            outs = [gemm(h, ta, tb, Ac, Bc, cm(C0, F64), 0.7, -1.3) for _, h in libs]
            same(f"{m}x{n}x{k} ta={ta} tb={tb} f32={fa}{fb}", outs)
for big, runs in ((66000, 256), (65537, 65)):
    rng = np.random.default_rng(big + runs)
    X, r = rng.standard_normal((runs, big)), 25
    Xu = CM(torch.as_tensor(X, device=dev), big, runs, big)
    W, Y = cm(rng.standard_normal((big, r)), F64), cm(rng.standard_normal((runs, r)), F64)
    for lay, Xc in (("padded", padded(X)), ("tight", Xu)):
        for kind, ta, tb, A, B, mo, no in (("tsk", 1, 0, Xc, W, runs, r),
                                           ("tsm", 0, 0, Xc, Y, big, r),
                                           ("tsm_t", 1, 1, Y, Xc, r, big)):
            outs = [gemm(h, ta, tb, A, B, CM.empty(mo, no, dev)) for _, h in libs]
            same(f"{kind} big={big} runs={runs} {lay}", outs)
if small_only:
    sys.exit(1 if bad else 0)


# ---- the four ensemble-streaming products of randomized_svd at the fit's shape ----------------
def timed(tag, call):
    """call(h) per library: warm-up, then WINDOWS windows of CALLS calls, libraries alternating."""
    for _, h in libs:
        for _ in range(WARM):
            call(h)
    torch.cuda.synchronize()
    ms = [[] for _ in libs]
    for _ in range(WINDOWS):
        for i, (_, h) in enumerate(libs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                call(h)
            e1.record()
            torch.cuda.synchronize()
            ms[i].append(e0.elapsed_time(e1) / CALLS)
    for i, (name, _) in enumerate(libs):
        verdict = "" if i == 0 else ("  holds" if np.median(ms[i]) <= max(ms[0]) else "  MISSED")
        print(f"time {tag:44s} {name:24s} median {np.median(ms[i]):7.4f} ms  range "
              f"{min(ms[i]):7.4f}-{max(ms[i]):7.4f} ({WINDOWS} windows x {CALLS}){verdict}",
              flush=True)


runs, ny, r = 512, 1_347_945, 25
gen = torch.Generator(device=dev).manual_seed(20240318)
Om = torch.randn((ny, r), generator=gen, device=dev, dtype=torch.float32)
Oc = CM.of_rowmajor(Om)                                   # (r x ny), as randomized_svd reads it
for ens in ("float32", "fp64 padded"):
    if ens == "float32":
        Xt = torch.randn((runs, ny), generator=gen, device=dev, dtype=torch.float32)
    else:
        ld = (ny + 15) // 16 * 16
        Xt = torch.full((runs, ld), float("nan"), dtype=F64, device=dev)[:, :ny]
        Xt.normal_(generator=gen)
    Xc = CM.of_rowmajor(Xt)                               # (ny x runs), ld = the row stride
    Ys = [CM.empty(runs, r, dev) for _ in libs]
    Zs = [CM.empty(r, ny, dev) for _ in libs]
    # each product's operands are the first library's outputs, so one difference shows once
    same(f"{ens}: Y = X Omega", [gemm(h, 1, 1, Xc, Oc, Y) for (_, h), Y in zip(libs, Ys)])
    timed(f"{ens}: Y = X Omega", lambda h: gemm(h, 1, 1, Xc, Oc, Ys[1]))
    Y0 = CM(Ys[0].t.clone(), runs, r, runs)
    same(f"{ens}: Zt = Y^T X", [gemm(h, 1, 1, Y0, Xc, Z) for (_, h), Z in zip(libs, Zs)])
    timed(f"{ens}: Zt = Y^T X", lambda h: gemm(h, 1, 1, Y0, Xc, Zs[1]))
    same(f"{ens}: Y = X Zt", [gemm(h, 1, 1, Xc, Zs[0], Y) for (_, h), Y in zip(libs, Ys)])
    timed(f"{ens}: Y = X Zt", lambda h: gemm(h, 1, 1, Xc, Zs[0], Ys[1]))
    Q = CM(Ys[0].t / Ys[0].t.norm(dim=1, keepdim=True), runs, r, runs)    # unit columns
    same(f"{ens}: B = Q^T X", [gemm(h, 1, 1, Q, Xc, Z) for (_, h), Z in zip(libs, Zs)])
    timed(f"{ens}: B = Q^T X", lambda h: gemm(h, 1, 1, Q, Xc, Zs[1]))
    del Xt, Xc, Ys, Zs, Y0, Q
    torch.cuda.empty_cache()
sys.exit(1 if bad else 0)
