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
