"""CPU tests of the drop-in boundary: libfo1hip.so loads, exports every symbol
include/fo1.h declares, and rejects bad arguments with the documented error codes
(no compute without a GPU)."""
import os
import re

import pytest

from vlm_fo1_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(header="fo1.h"):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fo1_[a-z0-9_]+)\s*\(", txt)))


def exported(so):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vlm_fo1_amd", so)], capture_output=True, text=True, check=True).stdout
    return sorted({l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("fo1_") and " T " in l})


def all_defined_dynamic_symbols(so):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vlm_fo1_amd", so)], capture_output=True, text=True, check=True).stdout
    return sorted({l.split()[-1] for l in out.splitlines() if l.strip()})


def test_export_table_is_exactly_the_headers():
    """nothing but the declared C entry points leaves the libraries — no un-prefixed helper, no mangled fo1:: internal,
    no kernel stub or kernel-handle object (-fvisibility=hidden + the headers' visibility pragma + csrc/exports.map)."""
    prod, ab = declared_symbols(), declared_symbols("fo1_ab.h")
    assert all_defined_dynamic_symbols("libfo1hip.so") == prod
    assert all_defined_dynamic_symbols("libfo1hip_ab.so") == sorted(prod + ab)


def test_library_exports_every_declared_symbol():
    lib = L.load()              # the test session's library: the PRODUCT build (tests/conftest.py)
    assert lib._name.endswith("libfo1hip.so")
    syms = declared_symbols()
    assert "fo1_hfre_region_pool" in syms
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/fo1.h but not exported"
    # and the Python binding table covers exactly the header
    assert sorted(L.SIGNATURES) == syms
    assert sorted(L.SIGNATURES_AB) == declared_symbols("fo1_ab.h")
    with L.use_ab() as ab:      # the test / bench build exports both headers; the switch routes L.load() and restores it afterwards
        assert L.load() is ab and L.ab_build() and ab._name.endswith("libfo1hip_ab.so")
        for sname in syms + sorted(L.SIGNATURES_AB):
            assert hasattr(ab, sname)
    assert L.load() is lib and not L.ab_build()


def test_product_library_has_no_switches_and_the_ab_build_has_exactly_the_two_headers():
    """the product library's export table IS include/fo1.h — none of the process-global A/B, ablation or
    tuning switches (include/fo1_ab.h) exist in it; the test / bench build exports both headers and nothing else."""
    prod, ab = declared_symbols(), declared_symbols("fo1_ab.h")
    assert not set(prod) & set(ab)
    assert exported("libfo1hip.so") == prod
    assert exported("libfo1hip_ab.so") == sorted(prod + ab)
    # fo1_ab.h = the process-global switches (`_set_`) + the measured no-gain kernel forms and instruments moved out of the product ABI in round 5
    extra = {"fo1_gemm_bf16_wtiled", "fo1_splitk_swiglu_bf16", "fo1_mfma_clock_probe", "fo1_gemm_profile_shapes", "fo1_traffic_probe"}
    assert all("_set_" in s or s in extra for s in ab) and extra <= set(ab) and not any("_set_" in s for s in prod)
    # the product build also leaves the measured-slower kernel forms out
    import subprocess
    for so, want in (("libfo1hip.so", False), ("libfo1hip_ab.so", True)):
        blob = open(os.path.join(ROOT, "vlm_fo1_amd", so), "rb").read()
        for kernel in (b"gemm_bt_p8_kernel", b"gemm_bt_p4p_kernel", b"attn_decode_wg_kernel", b"gemv_batch_kernel", b"hfre_pool_kernel", b"hfre_pool_bands_kernel"):
            assert (kernel in blob) == want, f"{kernel.decode()} {'missing from' if want else 'present in'} {so}"


def test_abi_version():
    assert L.load().fo1_abi_version() == 9


def test_hfre_argument_errors():
    lib = L.load()
    S = L.HfreSource
    ok = S(16, 120, 160, 256, 256, 120, 160, 0.25, 0, 0)
    arr = (S * 1)(ok)
    assert lib.fo1_hfre_workspace_bytes(arr, 1, 100) > 0
    # NULL boxes
    assert lib.fo1_hfre_region_pool(arr, 1, None, 3, None, 1.0, 1.0, 7, 0, 1.0, 1.0, None, 256, 256, None, 0, None) == -1
    assert b"NULL" in lib.fo1_last_error()
    # channel count not a multiple of 64
    bad = (S * 1)(S(16, 120, 160, 100, 104, 120, 160, 0.25, 0, 0))
    assert lib.fo1_hfre_region_pool(bad, 1, 16, 3, None, 1.0, 1.0, 7, 0, 1.0, 1.0, 16, 256, 256, None, 0, None) == -1
    # map larger than the LDS weight tables
    big = (S * 1)(S(16, 2000, 160, 256, 256, 2000, 160, 0.25, 0, 0))
    assert lib.fo1_hfre_workspace_bytes(big, 1, 1) == 0
    # zero boxes is a no-op, not an error
    assert lib.fo1_hfre_region_pool(arr, 1, None, 0, None, 1.0, 1.0, 7, 0, 1.0, 1.0, None, 256, 256, None, 0, None) == 0
    # workspace too small -> -2
    assert lib.fo1_hfre_region_pool(arr, 1, 16, 3, None, 1.0, 1.0, 7, 0, 1.0, 1.0, 16, 256, 256, 16, 8, None) == -2


def test_attention_argument_errors():
    """Every call is rejected before any HIP call (fake 4096-aligned integers stand for device pointers): the return code, the entry's prefix
    and the offending quantity in fo1_last_error(); n_items == 0 is a no-op.  The workspace sizes follow the documented partial layout,
    chunks x n_kv_heads x 16 x (head_dim + 2) x 4 bytes per sequence."""
    lib = L.load()
    P = [4096 * (i + 1) for i in range(8)]
    Q, K, VT, O, IT, WS, ST, PR = P

    def rejected(rc, want, prefix, *words):
        msg = lib.fo1_last_error()
        assert rc == want, (rc, msg)
        assert msg.startswith(prefix + b":") and all(w in msg for w in words), msg

    def fwd(**kw):      # fo1_attention_bf16: head dim 128, 4 query / 2 KV heads, one item, q_block 64
        a = dict(Q=Q, q_tok=512, q_head=128, K=K, k_tok=256, k_head=128, VT=VT, vt_row=64, O=O, o_tok=512, o_head=128, items=IT, n_items=1,
                 q_block=64, Hq=4, Hkv=2, hd=128, base=None)
        a.update(kw)
        return lib.fo1_attention_bf16(a["Q"], a["q_tok"], a["q_head"], a["K"], a["k_tok"], a["k_head"], a["VT"], a["vt_row"], a["O"], a["o_tok"],
                                      a["o_head"], a["items"], a["n_items"], a["q_block"], a["Hq"], a["Hkv"], a["hd"], 0.1, 1, a["base"], 0.0, None)

    rejected(fwd(K=None), -1, b"attention", b"NULL")
    rejected(fwd(Hq=3), -1, b"attention", b"head")
    rejected(fwd(hd=64), -1, b"attention", b"head_dim 64")
    rejected(fwd(q_block=48), -1, b"attention", b"q_block 48")
    rejected(fwd(q_tok=260), -1, b"attention", b"Q", b"stride")
    rejected(fwd(vt_row=66), -1, b"attention", b"V^T", b"stride")
    rejected(fwd(Q=Q + 8), -1, b"attention", b"misaligned")
    rejected(fwd(q_block=128, hd=32, q_head=32, k_head=32), -1, b"attention", b"q_block 128", b"head_dim")
    rejected(fwd(q_block=128, base=PR), -1, b"attention", b"q_block 128", b"q_row_base")
    rejected(fwd(q_block=128, n_items=70000), -1, b"attention", b"65535", b"70000")
    rejected(fwd(q_block=128, Hq=3, Hkv=3), -1, b"attention", b"even number of query heads")
    rejected(fwd(q_block=128, o_tok=260), -1, b"attention", b"q_block 128", b"O misaligned")
    rejected(fwd(q_block=128, k_tok=1 << 22), -1, b"attention", b"q_block 128", b"stride too large")
    assert fwd(n_items=0, K=None) == 0

    def win(**kw):      # fo1_attention_windows_bf16: head dim 80, 16 heads
        a = dict(Q=Q, K=K, k_tok=1280, VT=VT, O=O, o_tok=1280, o_rows=64, n_items=1, H=16, hd=80)
        a.update(kw)
        return lib.fo1_attention_windows_bf16(a["Q"], 1280, 80, a["K"], a["k_tok"], 80, a["VT"], 64, a["O"], a["o_tok"], 80, a["o_rows"], IT,
                                              a["n_items"], a["H"], a["H"], a["hd"], 0.1, 0.0, None)

    rejected(win(Q=None), -1, b"attention_windows", b"NULL")
    rejected(win(hd=128), -1, b"attention_windows", b"head dim", b"128")
    rejected(win(H=70000), -1, b"attention_windows", b"head")
    rejected(win(k_tok=260), -1, b"attention_windows", b"stride")
    rejected(win(VT=VT + 4), -1, b"attention_windows", b"misaligned")
    rejected(win(o_rows=0), -1, b"attention_windows", b"output")
    rejected(win(o_rows=1 << 21), -1, b"attention_windows", b"output", b"2 GiB")
    assert win(n_items=0, Q=None) == 0

    rejected(lib.fo1_attention_prefix_bf16(Q, 512, 128, K, 256, 128, VT, 64, O, 512, 128, IT, None, 1, 64, 4, 2, 128, 0.1, 1, 0.0, None),
             -1, b"attention_prefix", b"prefix_ranges")
    rejected(lib.fo1_attention_window_bias_bf16(Q, 192, 32, K, 192, 32, VT, 144, O, 192, 32, IT, 1, 64, 6, 32, 0.1, PR, 144, 12, 12, 1, 1, 0.0, None),
             -1, b"attention_window_bias", b"window geometry", b"shift=12")

    def dec(hd=128, ws_bytes=1 << 20):
        return lib.fo1_attention_decode_bf16(Q, K, 128, 128 * 644, VT, 644, O, ST, 640, 16, 2, hd, 0.1, WS, ws_bytes, None)

    rejected(dec(hd=64), -1, b"attention_decode", b"head_dim 64")
    rejected(dec(ws_bytes=16), -2, b"attention_decode", b"workspace")

    def dec_batch(q_seq=2048, Hq=16, ws_bytes=1 << 20):
        return lib.fo1_attention_decode_batch_bf16(Q, q_seq, K, 128, 128 * 2048, VT, 2048, O, 2048, ST, 3, 640, Hq, 2, 128, 0.1, WS, ws_bytes, None)

    rejected(dec_batch(ws_bytes=16), -2, b"attention_decode_batch", b"workspace")
    rejected(dec_batch(q_seq=1790), -1, b"attention_decode_batch", b"stride")
    rejected(dec_batch(Hq=34), -1, b"attention_decode_batch", b"16 query heads per KV head")

    per_chunk = 2 * 16 * (128 + 2) * 4          # bytes per chunk of one sequence: n_kv_heads x 16 rows x (head_dim + 2) floats
    assert lib.fo1_attention_decode_workspace_bytes(640, 2, 128) == 10 * per_chunk == 166400
    assert lib.fo1_attention_decode_batch_workspace_bytes(640, 2, 128, 3) == 3 * 10 * per_chunk == 499200
    assert lib.fo1_attention_decode_batch_workspace_bytes(640, 2, 128, 33) == 33 * 1 * per_chunk == 549120       # one 1024-key chunk
    assert lib.fo1_attention_decode_batch_workspace_bytes(2048, 2, 128, 64) == 64 * 2 * per_chunk == 2129920


def test_decode_linear_argument_errors():
    """fo1_gemv_bf16, fo1_gemv_batch_bf16 and fo1_gemv_attn_combine_bf16 reject every bad call before any HIP call (fake 4096-aligned
    integers stand for device pointers): the return code, the entry's prefix and the offending quantity in fo1_last_error() — the
    entries' own checks, then the dispatch refusals of the MFMA route (both builds) and of the v_dot2 route (test / bench build)."""
    lib = L.load()
    X, W, C, R, NW, COS, SIN, ST, KC, VT, PART = [4096 * (i + 1) for i in range(11)]

    def rejected(rc, prefix, *words, on=None):
        msg = (on or lib).fo1_last_error()
        assert rc == -1, (rc, msg)
        assert msg.startswith(prefix + b":") and all(w in msg for w in words), msg

    def gemv(**kw):     # fo1_gemv_bf16: one row of a 64 x 256 projection
        a = dict(x=X, ldx=256, W=W, ldw=256, res=None, C=C, M=1, N=64, K=256, act=0, norm=None)
        a.update(kw)
        return lib.fo1_gemv_bf16(a["x"], a["ldx"], a["W"], a["ldw"], None, a["res"], a["N"], a["C"], a["N"], a["M"], a["N"], a["K"], a["act"],
                                 a["norm"], 1e-6, None)

    rejected(gemv(x=None), b"gemv", b"NULL")
    rejected(gemv(W=None), b"gemv", b"NULL")
    rejected(gemv(C=None), b"gemv", b"NULL")
    rejected(gemv(M=0), b"gemv", b"bad shape", b"M=0")
    rejected(gemv(M=5), b"gemv", b"bad shape", b"M=5")
    rejected(gemv(K=12), b"gemv", b"bad shape", b"K=12")
    rejected(gemv(ldx=260), b"gemv", b"bad shape")
    rejected(gemv(ldw=260), b"gemv", b"bad shape")
    rejected(gemv(M=4, K=20000, ldx=20000, ldw=20000), b"gemv", b"does not fit LDS", b"M=4", b"K=20000")
    rejected(gemv(act=4), b"gemv", b"bad act")
    rejected(gemv(act=6), b"gemv", b"bad act")
    rejected(gemv(act=3, N=48), b"gemv", b"bad act/N")
    rejected(gemv(act=3, res=R), b"gemv", b"bad act/N")
    rejected(gemv(x=X + 8), b"gemv", b"misaligned")
    rejected(gemv(W=W + 8), b"gemv", b"misaligned")
    rejected(gemv(norm=NW + 8), b"gemv", b"misaligned")

    def batch(on=None, **kw):    # fo1_gemv_batch_bf16: one row of a 64 x 256 projection; mode 2: 2 query heads, 1 KV head
        a = dict(x=X, ldx=256, W=W, ldw=256, res=None, ldr=0, C=C, M=1, N=64, K=256, mode=0, norm=None, n_q=0, n_kv=0, cos=COS, sin=SIN,
                 state=ST, kc=KC, vt=VT)
        a.update(kw)
        return (on or lib).fo1_gemv_batch_bf16(a["x"], a["ldx"], a["W"], a["ldw"], None, a["res"], a["ldr"], a["C"], a["N"], a["M"], a["N"],
                                               a["K"], a["mode"], a["norm"], 1e-6, a["n_q"], a["n_kv"], a["cos"], a["sin"], a["state"],
                                               a["kc"], 128 * 64, a["vt"], 64, None)

    rejected(batch(x=None), b"gemv_batch", b"NULL")
    rejected(batch(W=None), b"gemv_batch", b"NULL")
    rejected(batch(C=None), b"gemv_batch", b"NULL")
    rejected(batch(M=0), b"gemv_batch", b"bad shape", b"M=0")
    rejected(batch(M=33), b"gemv_batch", b"bad shape", b"M=33")
    rejected(batch(K=12), b"gemv_batch", b"bad shape", b"K=12")
    rejected(batch(ldx=260), b"gemv_batch", b"bad shape")
    rejected(batch(ldw=260), b"gemv_batch", b"bad shape")
    rejected(batch(mode=3), b"gemv_batch", b"mode 3")
    rejected(batch(mode=-1), b"gemv_batch", b"mode -1")
    rejected(batch(x=X + 8), b"gemv_batch", b"misaligned")
    rejected(batch(W=W + 8), b"gemv_batch", b"misaligned")
    rejected(batch(norm=NW + 8), b"gemv_batch", b"misaligned")
    rejected(batch(mode=1, N=48), b"gemv_batch", b"SwiGLU", b"N % 32")
    rejected(batch(mode=1, res=R, ldr=64), b"gemv_batch", b"SwiGLU", b"no residual")
    qkv = dict(mode=2, n_q=2, n_kv=1, N=512)
    rejected(batch(**dict(qkv, N=384)), b"gemv_batch", b"QKV mode needs N")
    rejected(batch(**dict(qkv, n_kv=0, N=256)), b"gemv_batch", b"QKV mode needs N")
    for missing in ("cos", "sin", "state", "kc", "vt"):
        rejected(batch(**dict(qkv, **{missing: None})), b"gemv_batch", b"QKV mode operands")
    rejected(batch(**dict(qkv, res=R, ldr=512)), b"gemv_batch", b"QKV mode operands")
    # the MFMA route's refusals (no HIP call before them)
    rejected(batch(norm=NW, K=2112, ldx=2112, ldw=2112), b"gemv_batch", b"fused RMSNorm", b"K=2112")
    rejected(batch(M=17, mode=1, K=2112, ldx=2112, ldw=2112), b"gemv_batch", b"M > 16 with K > 2048", b"M=17", b"K=2112", b"mode=1")
    rejected(batch(M=17, N=8192, K=2112, ldx=2112, ldw=2112), b"gemv_batch", b"M > 16 with K > 2048", b"M=17", b"N=8192", b"K=2112")
    # operands the MFMA route cannot move four at a time: the product library has no other kernel
    assert lib._name.endswith("libfo1hip.so")
    rejected(batch(N=66), b"gemv_batch", b"operands must be 8-byte aligned", b"N=66")
    rejected(batch(res=R + 2, ldr=64), b"gemv_batch", b"operands must be 8-byte aligned")
    with L.use_ab() as ab:     # the v_dot2 route of the test / bench build
        try:
            assert ab.fo1_gemv_batch_set_impl(0) == 0
            rejected(batch(on=ab, M=9), b"gemv_batch", b"M <= 8", b"M=9", on=ab)
            rejected(batch(on=ab, M=8, norm=NW, K=8448, ldx=8448, ldw=8448), b"gemv_batch", b"fused RMSNorm", b"K=8448", b"M=8", on=ab)
            rejected(ab.fo1_gemv_batch_set_impl(2), b"gemv_batch_set_impl", b"2", on=ab)
            rejected(ab.fo1_gemv_batch_set_rows_per_lane(2), b"gemv_batch_set_rows_per_lane", b"2", on=ab)
        finally:
            assert ab.fo1_gemv_batch_set_impl(1) == 0

    def combine(**kw):  # fo1_gemv_attn_combine_bf16: 16 query / 2 KV heads (K = 2048), a 2048-feature o-projection
        a = dict(part=PART, state=ST, chunk=256, n_q=16, n_kv=2, W=W, ldw=2048, res=R, ldr=2048, C=C, ldc=2048, M=1, N=2048)
        a.update(kw)
        return lib.fo1_gemv_attn_combine_bf16(a["part"], 1 << 20, a["state"], a["chunk"], a["n_q"], a["n_kv"], a["W"], a["ldw"], a["res"], a["ldr"],
                                              a["C"], a["ldc"], a["M"], a["N"], None)

    for missing in ("part", "state", "W", "C"):
        rejected(combine(**{missing: None}), b"gemv_attn_combine", b"NULL")
    rejected(combine(M=0), b"gemv_attn_combine", b"M=0")
    rejected(combine(M=3), b"gemv_attn_combine", b"M=3")
    rejected(combine(n_kv=0), b"gemv_attn_combine", b"heads 16 / 0")
    rejected(combine(n_q=15), b"gemv_attn_combine", b"heads 15 / 2")
    rejected(combine(n_q=17, n_kv=1, ldw=2176), b"gemv_attn_combine", b"heads 17 / 1")
    rejected(combine(n_q=18, ldw=2304), b"gemv_attn_combine", b"heads 18 / 2", b"<= 2048")
    rejected(combine(N=4100, ldc=4100, ldr=4100), b"gemv_attn_combine", b"N=4100")
    rejected(combine(N=2046), b"gemv_attn_combine", b"N=2046")
    rejected(combine(chunk=96), b"gemv_attn_combine", b"bad layout")
    rejected(combine(chunk=0), b"gemv_attn_combine", b"bad layout")
    rejected(combine(ldw=2052), b"gemv_attn_combine", b"bad layout")
    rejected(combine(ldw=1024), b"gemv_attn_combine", b"bad layout")
    rejected(combine(W=W + 8), b"gemv_attn_combine", b"bad layout")
    rejected(combine(part=PART + 4), b"gemv_attn_combine", b"bad layout")
    rejected(combine(ldr=2050), b"gemv_attn_combine", b"residual / output layout")
    rejected(combine(ldr=1024), b"gemv_attn_combine", b"residual / output layout")
    rejected(combine(res=R + 4), b"gemv_attn_combine", b"residual / output layout")
    rejected(combine(ldc=1024), b"gemv_attn_combine", b"residual / output layout")


def test_vision_argument_errors():
    """The spatial operators of the towers, uniform and ragged (`_var`) entry of each, and the window-attention map pair: every bad call is
    rejected before any HIP call (fake 4096-aligned integers stand for device pointers) with the documented return code, the entry's own
    prefix (the `_var` entries say `_var`) and a word of the cause.  Where several checks could fire, the order is pinned."""
    lib = L.load()
    X, W9, B, Y, LW, LB, Hh, SG, WS = [4096 * (i + 1) for i in range(9)]
    TABLE = b"need a device fo1_img_seg table"

    def rejected(rc, prefix, *words, want=-1):
        msg = lib.fo1_last_error()
        assert rc == want, (rc, msg)
        assert msg.startswith(prefix + b":") and all(w in msg for w in words), msg

    def segs_checks(call, prefix):      # every ragged entry: NULL table, no image, more images than a grid dimension holds
        rejected(call(segs=None), prefix, TABLE)
        rejected(call(n=0), prefix, TABLE, b"1..65535")
        rejected(call(n=65536), prefix, TABLE, b"1..65535")

    def dwln(**kw):     # fo1_dwconv3x3_ln_bf16
        a = dict(x=X, w=W9, b=B, y=Y, lw=LW, lb=LB, h=Hh, H=5, W=7, C=64, batch=2)
        a.update(kw)
        return lib.fo1_dwconv3x3_ln_bf16(a["x"], a["w"], a["b"], a["y"], a["lw"], a["lb"], 1e-5, a["h"], a["H"], a["W"], a["C"], a["batch"], None)

    for missing in ("x", "w", "b", "y", "lw", "lb", "h"):
        rejected(dwln(**{missing: None}), b"dwconv_ln", b"NULL")
    rejected(dwln(y=X), b"dwconv_ln", b"aliased")
    rejected(dwln(h=X), b"dwconv_ln", b"aliased")
    rejected(dwln(h=Y), b"dwconv_ln", b"aliased")
    rejected(dwln(x=None, C=12), b"dwconv_ln", b"NULL")           # operands before shape
    rejected(dwln(C=12), b"dwconv_ln", b"bad shape", b"5x7x12")
    rejected(dwln(C=2056), b"dwconv_ln", b"bad shape", b"C <= 2048")
    rejected(dwln(C=0), b"dwconv_ln", b"bad shape")
    rejected(dwln(H=0), b"dwconv_ln", b"bad shape")
    rejected(dwln(W=0), b"dwconv_ln", b"bad shape")
    rejected(dwln(batch=0), b"dwconv_ln", b"bad shape")
    rejected(dwln(H=1 << 20, W=1 << 14, C=256, batch=1), b"dwconv_ln", b"too many pixel runs")

    def dwln_var(**kw):     # fo1_dwconv3x3_ln_var_bf16
        a = dict(x=X, w=W9, b=B, y=Y, lw=LW, lb=LB, h=Hh, segs=SG, n=2, max=35, total=60, C=64)
        a.update(kw)
        return lib.fo1_dwconv3x3_ln_var_bf16(a["x"], a["w"], a["b"], a["y"], a["lw"], a["lb"], 1e-5, a["h"], a["segs"], a["n"], a["max"], a["total"],
                                             a["C"], None)

    for missing in ("x", "w", "b", "y", "lw", "lb", "h"):
        rejected(dwln_var(**{missing: None}), b"dwconv_ln_var", b"NULL")
    rejected(dwln_var(y=X), b"dwconv_ln_var", b"aliased")
    rejected(dwln_var(h=X), b"dwconv_ln_var", b"aliased")
    rejected(dwln_var(h=Y), b"dwconv_ln_var", b"aliased")
    rejected(dwln_var(x=None, segs=None), b"dwconv_ln_var", b"NULL operand")      # operands, then the table, then the shape
    segs_checks(dwln_var, b"dwconv_ln_var")
    rejected(dwln_var(segs=None, C=12), b"dwconv_ln_var", TABLE)
    rejected(dwln_var(C=12), b"dwconv_ln_var", b"bad shape")
    rejected(dwln_var(C=2056), b"dwconv_ln_var", b"bad shape", b"C <= 2048")
    rejected(dwln_var(max=0), b"dwconv_ln_var", b"bad shape")

    def im2col(**kw):       # fo1_im2col_bf16: a 3 x 3 / stride 2 / pad 1 embed of a 9 x 11 x 16 map
        a = dict(x=X, col=Y, H=9, W=11, C=16, KH=3, KW=3, stride=2, pad=1, ld=144, batch=2)
        a.update(kw)
        return lib.fo1_im2col_bf16(a["x"], a["col"], a["H"], a["W"], a["C"], a["KH"], a["KW"], a["stride"], a["pad"], a["ld"], a["batch"], None)

    rejected(im2col(x=None), b"im2col", b"NULL")
    rejected(im2col(col=None), b"im2col", b"NULL")
    rejected(im2col(x=None, C=12), b"im2col", b"NULL")
    rejected(im2col(C=12), b"im2col", b"bad parameters")
    rejected(im2col(stride=0), b"im2col", b"bad parameters")
    rejected(im2col(KH=0), b"im2col", b"bad parameters")
    rejected(im2col(pad=-1), b"im2col", b"bad parameters")
    rejected(im2col(C=12, ld=8), b"im2col", b"bad parameters")          # parameters before the output shape
    rejected(im2col(ld=136), b"im2col", b"bad output shape")            # smaller than KH * KW * C
    rejected(im2col(ld=148), b"im2col", b"bad output shape")            # not a multiple of 8
    rejected(im2col(batch=0), b"im2col", b"bad output shape")
    rejected(im2col(H=0, pad=0), b"im2col", b"bad output shape")

    def im2col_var(**kw):   # fo1_im2col_var_bf16
        a = dict(x=X, col=Y, segs=SG, n=2, max=30, total=50, C=16, KH=3, KW=3, stride=2, pad=1, ld=144)
        a.update(kw)
        return lib.fo1_im2col_var_bf16(a["x"], a["col"], a["segs"], a["n"], a["max"], a["total"], a["C"], a["KH"], a["KW"], a["stride"], a["pad"],
                                       a["ld"], None)

    rejected(im2col_var(x=None), b"im2col_var", b"NULL")
    rejected(im2col_var(col=None), b"im2col_var", b"NULL")
    rejected(im2col_var(x=None, segs=None), b"im2col_var", b"NULL")
    segs_checks(im2col_var, b"im2col_var")
    rejected(im2col_var(segs=None, C=12), b"im2col_var", TABLE)
    rejected(im2col_var(C=12), b"im2col_var", b"bad parameters")
    rejected(im2col_var(stride=0), b"im2col_var", b"bad parameters")
    rejected(im2col_var(ld=136), b"im2col_var", b"bad parameters")
    rejected(im2col_var(ld=148), b"im2col_var", b"bad parameters")
    rejected(im2col_var(max=0), b"im2col_var", b"bad parameters")

    def one_check(entry, var_entry, prefix, operands, extent):
        """The copy-like operators make one check of the operands and the shape, the ragged twin then the table.
        -> (uniform(**kw), ragged(**kw)); `extent` = the uniform entry's trailing shape arguments after (H, W)."""
        def uni(**kw):
            a = dict(p=list(operands), H=13, W=17, C=64, ws=12, batch=2)
            a.update(kw)
            return getattr(lib, entry)(*a["p"], a["H"], a["W"], *[a[k] for k in extent], a["batch"], None)

        def var(**kw):
            a = dict(p=list(operands), segs=SG, n=2, max=288, total=576, C=64, ws=12)
            a.update(kw)
            return getattr(lib, var_entry)(*a["p"], a["segs"], a["n"], a["max"], a["total"], *[a[k] for k in extent], None)

        for i in range(len(operands)):
            nulled = [None if j == i else p for j, p in enumerate(operands)]
            rejected(uni(p=nulled), prefix, b"bad arguments")
            rejected(var(p=nulled), prefix + b"_var", b"bad arguments")
        rejected(uni(C=12), prefix, b"bad arguments")
        rejected(uni(batch=0), prefix, b"bad arguments")
        rejected(var(C=12), prefix + b"_var", b"bad arguments")
        rejected(var(max=0), prefix + b"_var", b"bad arguments")
        rejected(var(C=12, segs=None), prefix + b"_var", b"bad arguments")      # operands and shape before the table
        segs_checks(var, prefix + b"_var")
        return uni, var

    uni, var = one_check("fo1_window_partition_bf16", "fo1_window_partition_var_bf16", b"window_partition", (X, Y), ("C", "ws"))
    rejected(uni(ws=0), b"window_partition", b"bad arguments")
    rejected(var(ws=0), b"window_partition_var", b"bad arguments")
    uni, var = one_check("fo1_window_reverse_add_bf16", "fo1_window_reverse_add_var_bf16", b"window_reverse", (X, B, Y), ("C", "ws"))
    rejected(uni(ws=0), b"window_reverse", b"bad arguments")
    rejected(var(ws=0), b"window_reverse_var", b"bad arguments")
    uni, var = one_check("fo1_pixel_shuffle2_bf16", "fo1_pixel_shuffle2_var_bf16", b"pixel_shuffle", (X, Y), ("C",))
    rejected(uni(C=0), b"pixel_shuffle", b"bad arguments")
    rejected(var(C=0), b"pixel_shuffle_var", b"bad arguments")
    uni, var = one_check("fo1_maxpool2_bf16", "fo1_maxpool2_var_bf16", b"maxpool", (X, Y), ("C",))
    rejected(uni(H=1), b"maxpool", b"bad arguments")
    rejected(uni(W=1), b"maxpool", b"bad arguments")

    def chattn(**kw):       # fo1_channel_attention_bf16: 2 images of 221 tokens, 64 channels
        a = dict(qkv=X, ld=192, N=221, C=64, out=Y, ldo=64, batch=2, ws=WS, bytes=lib.fo1_channel_attention_workspace_bytes(221, 64, 2))
        a.update(kw)
        return lib.fo1_channel_attention_bf16(a["qkv"], a["ld"], a["N"], a["C"], a["out"], a["ldo"], a["batch"], a["ws"], a["bytes"], None)

    def chattn_var(**kw):   # fo1_channel_attention_var_bf16: 2 images, the larger of 300 tokens
        a = dict(qkv=X, ld=192, segs=SG, n=2, max=300, total=521, C=64, out=Y, ldo=64, ws=WS,
                 bytes=lib.fo1_channel_attention_var_workspace_bytes(300, 64, 2))
        a.update(kw)
        return lib.fo1_channel_attention_var_bf16(a["qkv"], a["ld"], a["segs"], a["n"], a["max"], a["total"], a["C"], a["out"], a["ldo"], a["ws"],
                                                  a["bytes"], None)

    assert lib.fo1_channel_attention_workspace_bytes(221, 64, 2) > 0
    assert lib.fo1_channel_attention_var_workspace_bytes(300, 64, 2) == lib.fo1_channel_attention_workspace_bytes(300, 64, 2)
    for call, prefix, size in ((chattn, b"channel_attention", "N"), (chattn_var, b"channel_attention_var", "max")):
        for missing in ("qkv", "out", "ws"):
            rejected(call(**{missing: None}), prefix, b"NULL")
        rejected(call(qkv=None, C=48), prefix, b"NULL")
        rejected(call(C=48, ld=144, ldo=48), prefix, b"bad shape")          # C % 32
        rejected(call(C=0), prefix, b"bad shape")
        rejected(call(**{size: 0}), prefix, b"bad shape")
        rejected(call(ld=184), prefix, b"bad shape")                        # ld < 3 C
        rejected(call(ld=196), prefix, b"bad shape")                        # ld % 8
        rejected(call(ldo=56), prefix, b"bad shape")                        # ldo < C
        rejected(call(C=48, ldo=68), prefix, b"bad shape")                  # the shape before the alignment
        rejected(call(ldo=68), prefix, b"16-byte aligned", b"ldo % 8")
        rejected(call(qkv=X + 8), prefix, b"16-byte aligned")
        rejected(call(out=Y + 8), prefix, b"16-byte aligned")
        rejected(call(ldo=68, bytes=16), prefix, b"16-byte aligned")        # the alignment before the workspace
        rejected(call(bytes=0), prefix, b"workspace too small", want=-2)
    rejected(chattn(bytes=lib.fo1_channel_attention_workspace_bytes(221, 64, 2) - 1), b"channel_attention", b"workspace too small", want=-2)
    rejected(chattn_var(bytes=lib.fo1_channel_attention_var_workspace_bytes(300, 64, 2) - 1), b"channel_attention_var", b"workspace too small",
             want=-2)
    rejected(chattn(batch=0), b"channel_attention", b"bad shape", b"N=221 C=64")
    rejected(chattn_var(qkv=None, segs=None), b"channel_attention_var", b"NULL")     # operands, the table, the shape
    segs_checks(chattn_var, b"channel_attention_var")
    rejected(chattn_var(segs=None, C=48), b"channel_attention_var", TABLE)

    def wmap(**kw):         # fo1_window_attention_map_bf16: 2 images of 13 x 17 pixels, 2 heads
        a = dict(qkv=X, ld=192, C=64, heads=2, window=12, H=13, W=17, batch=2, pad=B, out=Y, ldo=64)
        a.update(kw)
        return lib.fo1_window_attention_map_bf16(a["qkv"], a["ld"], a["C"], a["heads"], a["window"], a["H"], a["W"], a["batch"], a["pad"], a["out"],
                                                 a["ldo"], 0.1, None)

    def wmap_var(**kw):     # fo1_window_attention_map_var_bf16
        a = dict(qkv=X, ld=192, C=64, heads=2, window=12, segs=SG, n=2, max=4, total=521, pad=B, out=Y, ldo=64)
        a.update(kw)
        return lib.fo1_window_attention_map_var_bf16(a["qkv"], a["ld"], a["C"], a["heads"], a["window"], a["segs"], a["n"], a["max"], a["total"],
                                                     a["pad"], a["out"], a["ldo"], 0.1, None)

    rejected(wmap(H=0), b"window_attention_map", b"bad shape 0x17 x2")
    rejected(wmap(batch=0), b"window_attention_map", b"bad shape")
    rejected(wmap(batch=0, qkv=None), b"window_attention_map", b"bad shape")         # the entry's own shape check comes first
    rejected(wmap_var(segs=None), b"window_attention_map_var", b"fo1_img_seg table")
    rejected(wmap_var(segs=None, qkv=None), b"window_attention_map_var", b"fo1_img_seg table")
    assert wmap_var(n=0, qkv=None) == 0 and wmap_var(total=0, qkv=None) == 0         # nothing to do is not an error
    rejected(wmap_var(n=65536), b"window_attention_map_var", b"65536 images")
    rejected(wmap_var(max=0), b"window_attention_map_var", b"0 windows per image")
    for call, prefix in ((wmap, b"window_attention_map"), (wmap_var, b"window_attention_map_var")):
        for missing in ("qkv", "out", "pad"):
            rejected(call(**{missing: None}), prefix, b"NULL")
        rejected(call(qkv=None, heads=3), prefix, b"NULL")
        rejected(call(heads=3), prefix, b"head dim 32", b"C=64, 3 heads")
        rejected(call(heads=3, window=7), prefix, b"head dim 32")
        rejected(call(window=7), prefix, b"12 x 12 windows", b"got 7")
        rejected(call(ld=184), prefix, b"16-byte aligned")
        rejected(call(ldo=68), prefix, b"16-byte aligned")
        rejected(call(pad=B + 8), prefix, b"16-byte aligned")
    rejected(wmap(batch=70000), b"window_attention_map", b"70000 images")
    rejected(wmap(H=4000, W=4000), b"window_attention_map", b"windows per image")
    rejected(wmap(H=12 * 255, W=12 * 255, batch=600, ldo=1 << 16), b"window_attention_map", b"2 GiB")


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "nope.so"))
    monkeypatch.setattr(L, "LIB_PATH_AB", str(tmp_path / "nope_ab.so"))
    with pytest.raises(L.Fo1Error):
        L.load()


def test_plain_c_host_builds_against_the_header_and_drives_the_library(tmp_path):
    """include/fo1.h is valid C99 (a non-Python integrator's compiler sees it), and a C program with no Python / torch in the process
    loads the library, sizes a workspace and gets an argument error back as (rc < 0, fo1_last_error() text) — tests/host_emul/abi_host.c."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    inc = os.path.join(root, "include")
    hdr = tmp_path / "hdr.c"
    hdr.write_text('#include "fo1.h"\n#include "fo1_ab.h"\nint main(void) { return 0; }\n')
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, "-fsyntax-only", str(hdr)], check=True)
    exe = tmp_path / "abi_host"
    subprocess.run([gcc, "-std=c99", "-Wall", "-I", inc, os.path.join(root, "tests", "host_emul", "abi_host.c"), "-o", str(exe), "-ldl"], check=True)
    so = os.path.join(root, "vlm_fo1_amd", "libfo1hip.so")
    r = subprocess.run([str(exe), so], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rc=-1" in r.stdout and "NULL boxes" in r.stdout
