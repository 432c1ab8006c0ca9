"""gl3_kv_seq_copy (prefix fork) without a GPU: the symbol is declared, exported and bound, the header stays strict C99, and
tools/gl3_batch_run knows --share-prefix."""
import os
import re
import subprocess

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gpullama3_hip.h")
EXE = os.path.join(ROOT, "tools", "gl3_batch_run")


def test_symbol_is_exported_and_bound(pkg):
    from importlib import import_module
    hip = import_module(ge.PKG_NAME + ".hip")
    assert "gl3_kv_seq_copy" in hip.check_exports()
    assert hasattr(import_module(ge.PKG_NAME + ".plan").HipMasterPlan, "kv_seq_copy")


def test_header_declares_it():
    hdr = open(HEADER).read()
    assert re.search(r"GL3_API\s+int32_t\s+gl3_kv_seq_copy\s*\(\s*gl3_ctx\s*\*\s*ctx,\s*int32_t\s+src_seq,\s*const\s+int32_t\s*\*\s*dst_seqs,"
                     r"\s*int32_t\s+n_dst,\s*int32_t\s+p0,\s*int32_t\s+p1\s*\)\s*;", hdr)


def test_header_is_still_plain_c99(tmp_path):
    """The gcc line of test_lib_loads.py, on a translation unit that names the new entry."""
    src = tmp_path / "t.c"
    src.write_text('#include "gpullama3_hip.h"\n'
                   'int main(void) { int32_t (*f)(gl3_ctx*, int32_t, const int32_t*, int32_t, int32_t, int32_t) = gl3_kv_seq_copy; (void)f; return GL3_OK; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_tool_accepts_share_prefix():
    """--share-prefix alone is a known flag: the complaint is about the missing model and prompts, not about the argument."""
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ge.PKG_DIR, "csrc"), "../../tools/gl3_batch_run"])
    r = subprocess.run([EXE, "--share-prefix"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "-m model.gguf and --prompts file are required" in r.stderr and "unknown argument" not in r.stderr
