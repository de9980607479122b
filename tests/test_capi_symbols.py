"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/rb_capi.h declares; calls that need a device fail loudly (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "rb_capi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rb_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from rnabloom import _native as N
    lib = C.CDLL(N.LIB_PATH)
    names = declared_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), "librb_hip.so does not export %s" % n
    bound = {s[0] for s in N.SYMBOLS}
    assert set(names) == bound, set(names) ^ bound


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from rnabloom import _native as N
    p = N.GraphParams(1000, 1000, 1000, 2, 2, 2, 25, 0, 1, 0, 0, 0, 0)
    h = C.c_void_p()
    rc = N.lib.rb_graph_create(C.byref(p), C.byref(h))
    assert rc != 0 and b"hipGetDeviceCount" in N.lib.rb_last_error()
    b = C.c_void_p()
    assert N.lib.rb_batch_create_ascii(0, None, None, None, 0, 3, C.byref(b)) != 0


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, "rna-bloom_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                txt = open(os.path.join(dp, f), errors="replace").read()
                assert "rb_oracle" not in txt.replace("oracle/rb_oracle.c rbo_rng31", "") or f.endswith(".hpp"), f
                assert "import rbo" not in txt and "from oracle" not in txt, f


def test_no_device_resource_owner_has_static_storage():
    """DevBuf, Stream, Event, HostBuf and BatchPtr (csrc/rb_internal.hpp) release in their destructors; one with static, thread or namespace
    storage would call hipFree / hip*Destroy after the runtime has shut down at process exit, which crashes.  Owners live in handles and scopes."""
    owner = r"(?:rb::)?(?:DevBuf|Stream|Event|HostBuf<[^>]*>|BatchPtr)"
    csrc = os.path.join(ROOT, "rna-bloom_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        txt = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f), errors="replace").read())
        hits = re.findall(r"^[ \t]*(?:static|thread_local)\b[^;(]*\b%s(?!\w)[^;(]*;" % owner, txt, flags=re.M)      # static / thread_local, any scope
        hits += re.findall(r"^%s\s+\w+\s*[;={\[,]" % owner, txt, flags=re.M)                                     # column 0: namespace scope
        assert not hits, (f, hits)


def test_expected_size_matches_reference_formula():
    from rnabloom import _native as N
    import math
    for n, fpr, h in [(16_500_000, 0.01, 2), (450_000_000, 0.01, 2), (1000, 0.05, 3), (10 ** 9, 0.01, 1)]:
        f32 = C.c_float(fpr).value
        r = -h / math.log(1 - math.exp(math.log(f32) / h))
        assert N.lib.rb_expected_size(n, fpr, h) == math.ceil(n * r)


# ---- the JNI layer as source (jni/rb_jni.c, java/rnabloom/graph/NativeGraph.java): no JDK in the image, so it is
#      checked structurally and type-checked against the JNI declarations the shim uses ----
def _jni_functions():
    src = open(os.path.join(ROOT, "jni", "rb_jni.c")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\bFN\((\w+)\)\s*\(", src):
        depth, i = 0, src.index("{", m.end())
        j = i
        while True:
            depth += src[j] == "{"; depth -= src[j] == "}"
            j += 1
            if depth == 0: break
        out[m.group(1)] = src[i:j]
    return out


def test_every_native_method_has_a_jni_function_that_calls_the_c_abi():
    java = open(os.path.join(ROOT, "java", "rnabloom", "graph", "NativeGraph.java")).read()
    java = re.sub(r"/\*.*?\*/", "", java, flags=re.S)
    natives = re.findall(r"public static native [\w\[\]]+ (\w+)\(", java)
    fns = _jni_functions()
    assert len(natives) >= 45 and sorted(natives) == sorted(fns), set(natives) ^ set(fns)
    from rnabloom import _native as N
    exported = {s[0] for s in N.SYMBOLS}
    called = set()
    for name, body in fns.items():
        hits = set(re.findall(r"\b(rb_[a-z0-9_]+)\s*\(", body))
        assert hits and hits <= exported, (name, hits - exported)
        called |= hits
    # everything a single-process host needs is reachable from Java (the rb_shard_* phases belong to the multi-GPU driver)
    missing = {s for s in exported - called if not s.startswith("rb_shard_") and s not in (
        "rb_last_error", "rb_build_id", "rb_graph_create_shard", "rb_graph_profile_enable", "rb_graph_profile_get", "rb_batch_create_synthetic", "rb_debug_probe_cbf", "rb_debug_scan_u32", "rb_debug_sort_pairs", "rb_debug_group", "rb_debug_select",
        "rb_debug_cache_export", "rb_debug_prefilter",
        "rb_batch_download_ascii", "rb_nthash_batch", "rb_graph_add_batch")}
    assert not missing, missing


def test_jni_shim_type_checks_against_the_jni_declarations_it_uses():
    import shutil, subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "tests", "jni_stub"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "jni", "rb_jni.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the Java drop-in classes as source (java/rnabloom/{graph,bloom}/*.java): every public constructor and method of the
#      reference classes the boundary keeps exists with the same name and parameter types; the list is a
#      fixture made from the reference by tests/golden/gen_java_api.py (names and types only) ----
def _java_public_methods(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = set()
    for m in re.finditer(r"\bpublic\s+((?:static\s+|final\s+|synchronized\s+)*)([\w<>\[\], ]+?\s+)?(\w+)\s*\(([^)]*)\)\s*(?:throws [\w, .]+)?\s*\{", text):
        params = tuple(re.sub(r"\bfinal\s+", "", p).strip().rsplit(None, 1)[0].replace(" ", "") for p in m.group(4).split(",") if p.strip())
        out.add((m.group(3), params, "static" in m.group(1)))
    return out


def test_java_drop_in_classes_keep_every_public_signature_of_the_reference():
    import json
    api = json.load(open(os.path.join(ROOT, "tests", "golden", "java_api.json")))
    where = {"BloomFilterDeBruijnGraph": "graph", "BloomFilter": "bloom", "CountingBloomFilter": "bloom", "PairedKeysBloomFilter": "bloom",
             "Kmer": "graph", "CanonicalKmer": "graph"}
    natives = set(re.findall(r"public static (?:native )?[\w\[\]]+ (\w+)\(", open(os.path.join(ROOT, "java", "rnabloom", "graph", "NativeGraph.java")).read()))
    for cls, pkg in where.items():
        src = open(os.path.join(ROOT, "java", "rnabloom", pkg, cls + ".java")).read()
        have = _java_public_methods(src)
        if cls == "CanonicalKmer":              # a subclass: the public methods it does not override are Kmer's (constructors are never inherited)
            assert re.search(r"public class CanonicalKmer extends Kmer\b", src)
            kmer_src = open(os.path.join(ROOT, "java", "rnabloom", "graph", "Kmer.java")).read()
            have |= {m for m in _java_public_methods(kmer_src) if m[0] != "Kmer"}
        want = {(m["name"], tuple(m["params"]), m["static"]) for m in api[cls]}
        assert len(want) >= 15
        missing = want - have
        assert not missing, (cls, sorted(missing))
        # ... and the class really goes through the JNI surface: every NativeGraph member it names exists
        used = set(re.findall(r"NativeGraph\.(\w+)\(", src))
        assert (used or cls == "CanonicalKmer") and used <= natives, (cls, used - natives)
    # the hottest query of the reference (graph.getKmers: 18 call sites) goes through the BATCHED native, not through one getCount per k-mer
    g = open(os.path.join(ROOT, "java", "rnabloom", "graph", "BloomFilterDeBruijnGraph.java")).read()
    g = re.sub(r"/\*.*?\*/", "", g, flags=re.S)
    assert "hashFunction.getKmers(" not in g
    prof = g[g.index("private WindowProfile profile("):]
    assert "NativeGraph.getKmers(handle" in prof[:prof.index("\n    }\n")]
    for sig in ("public ArrayList<Kmer> getKmers(String seq)", "public ArrayList<Kmer> getKmers(String seq, int start, int end)",
                "public ArrayList<Kmer> getKmers(String seq, float minCoverage)"):
        body = g[g.index(sig):]
        body = body[:body.index("\n    }\n") if "\n    }\n" in body[:4000] and body.index("{") < body.index("\n") and not body[:body.index("\n")].rstrip().endswith("}") else body.index("\n")]
        assert "profile(" in body or "getKmers(seq, 0, seq.length())" in body, sig
    # the variants and isValidSeq are one batched lookup each
    for name in ("endVariants", "isValidSeq"):
        body = g[g.index(name + "("):]
        assert "NativeGraph.contains(handle" in body[:body.index("\n    }\n")], name
    # the neighbour-extension inner loop: a k-mer's neighbourhood is ONE native call (the reference: four graph.getCount calls), and no method of
    # the two classes falls back to the per-candidate iterators of the reference
    km = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "java", "rnabloom", "graph", "Kmer.java")).read(), flags=re.S)
    assert km.count("NativeGraph.neighbors(") == 1 and "NTHashIterator" not in km
    ck = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "java", "rnabloom", "graph", "CanonicalKmer.java")).read(), flags=re.S)
    assert "NTHashIterator" not in ck and "protected long reverseHashForNative()" in ck
    worker = open(os.path.join(ROOT, "java", "rnabloom", "graph", "NativeFastqToGraphWorker.java")).read()
    assert "NativeGraph.addReads(" in worker and "implements Runnable" in worker


# ---- occupancy budget of the hot kernels, read from the code objects inside librb_hip.so (no GPU needed) ----
def _kernel_resources():
    """{demangled-ish kernel name: (vgprs, spilled vgprs, LDS bytes)} of every gfx950 kernel bundled in the library"""
    import struct, subprocess, tempfile
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("no llvm-readelf")
    data = open(os.path.join(ROOT, "rna-bloom_amd", "lib", "librb_hip.so"), "rb").read()
    out, at = {}, 0
    while True:
        at = data.find(b"__CLANG_OFFLOAD_BUNDLE__", at)
        if at < 0:
            break
        n = struct.unpack_from("<Q", data, at + 24)[0]
        o = at + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, o); o += 24
            triple = data[o:o + tl]; o += tl
            if b"gfx950" in triple and size:
                with tempfile.NamedTemporaryFile(suffix=".co") as f:
                    f.write(data[at + off: at + off + size]); f.flush()
                    txt = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True).stdout
                for blk in txt.split("- .agpr_count")[1:] if "- .agpr_count" in txt else txt.split("    - ")[1:]:
                    nm = re.search(r"\.name:\s+(\S+)", blk); vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
                    sp = re.search(r"\.vgpr_spill_count:\s+(\d+)", blk); lds = re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk)
                    if nm and vg:
                        out[nm.group(1)] = (int(vg.group(1)), int(sp.group(1)) if sp else 0, int(lds.group(1)) if lds else 0)
        at += 24
    return out


def test_hot_kernels_keep_their_occupancy_budget():
    """k_group_buckets<512> runs two workgroups of 512 threads per CU = 4 wavefronts per SIMD, which needs <= 128 VGPRs: round 4 saw 132 after
    an innocent addition and the kernel went from 25 to 39 ms per step (one workgroup per CU).  The register counts are in the code
    objects: checked here, without a GPU, together with "no spills" for the kernels the step time is made of."""
    res = _kernel_resources()
    assert len(res) > 100, len(res)
    pick = lambda frag: {k: v for k, v in res.items() if frag in k}
    gb = pick("k_group_bucketsILi512E")
    assert len(gb) == 2 and all(v[0] <= 128 and v[1] == 0 for v in gb.values()), gb
    assert all(v[2] <= 80 * 1024 for v in gb.values()), gb                         # two workgroups share the CU's 160 KB of LDS
    for frag in ("k_filter_reads_pipe", "k_part_scatterILi512E", "k_part_countILi512E", "k_probe_h2", "k_resolve_apply", "k_hash_windows_resume", "k_pairs_reads"):
        ks = pick(frag)
        assert ks and all(v[1] == 0 for v in ks.values()), (frag, ks)
    ps = pick("k_part_scatterILi512ELi8E")
    assert all(v[0] <= 64 and v[2] <= 53 * 1024 + 512 for v in ps.values()), ps     # three workgroups per CU (DESIGN s5)
    sw = pick("k_sweep_bitsILi512E")
    assert sw and all(v[0] <= 128 for v in sw.values()), sw                           # swept Bloom-bit stage: two workgroups of 512 threads per CU (a few spilled registers are the price)
    so = pick("k_scan_one")
    assert so and all(v[2] <= 40 * 1024 for v in so.values()), so                      # single-workgroup scans must fit beside three bucket workgroups of 40 KB (DESIGN s5 "Round 4")


# ---- the k_pairs_insert miscompile (DESIGN s5): a kernel that picked its store target at run time inside a rolled loop was exact on every
#      small test and set 2 % of its bits at wrong places once a SIMD held more than one of its wavefronts (hipcc 7.2 -O3, gfx950).  Which
#      instruction sequence goes wrong was never isolated, so the pattern is fenced instead: no kernel may contain it. ----
def _blank(m):
    return re.sub(r"[^\n]", " ", m.group(0))


def _match_close(s, i, o, c):
    d = 0
    while True:
        d += s[i] == o; d -= s[i] == c; i += 1
        if d == 0:
            return i


def _stmt_end(s, i):
    """end of the statement that starts at s[i]: a block, or up to the ';' at nesting depth 0; an if carries its else along"""
    while s[i].isspace():
        i += 1
    if s[i] == "{":
        return _match_close(s, i, "{", "}")
    m = re.match(r"(if|for|while)\b\s*", s[i:])
    if m:
        j = _stmt_end(s, _match_close(s, i + m.end(), "(", ")"))
        if m.group(1) == "if":
            e = re.match(r"\s*else\b", s[j:])
            if e:
                j = _stmt_end(s, j + e.end())
        return j
    d = 0
    while True:
        c = s[i]
        d += c in "({["; d -= c in ")}]"
        i += 1
        if c == ";" and d == 0:
            return i


def _stores(txt):
    return bool(re.search(r"\b\w+\s*\[[^;]*?\]\s*(?:[|&^+\-]?=)[^=]", txt) or re.search(r"\b(atomic\w+|bit_set|__hip_atomic\w+)\s*\(", txt))


def run_time_store_target_choices(src):
    """[(kernel, pointer, line)]: inside a loop of a __global__ function, `if (p) { ...store... } else { ...store... }` with p one of the
    kernel's writable pointer parameters — the choice between two store targets made per iteration instead of per instantiation"""
    src = re.sub(r"/\*.*?\*/", _blank, src, flags=re.S)
    src = re.sub(r"//[^\n]*", _blank, src)
    src = re.sub(r"#ifdef RB_DIAG_PAIRS.*?#endif", _blank, src, flags=re.S)       # the failing form itself, kept as the reproducer (never built by default)
    hits = []
    for m in re.finditer(r"__global__\s+void\s*(?:__launch_bounds__\s*\([^)]*\)\s*)?(\w+)\s*\(", src):
        i = _match_close(src, m.end() - 1, "(", ")")
        if not re.match(r"\s*\{", src[i:]):
            continue
        params, j = src[m.end():i - 1], src.index("{", i)
        body, line0 = src[j:_match_close(src, j, "{", "}")], src.count("\n", 0, j) + 1
        ptrs = [mm.group(2) for p in params.split(",") for mm in [re.match(r"(.*?)\*\s*(?:__restrict__\s*)?(\w+)$", p.strip())] if mm and "const" not in mm.group(1)]
        loops = []
        for lm in re.finditer(r"\b(for|while)\s*\(", body):
            e = _match_close(body, lm.end() - 1, "(", ")")
            if not re.match(r"\s*;", body[e:]):                  # (the tail of a do-while has no body)
                loops.append((e, _stmt_end(body, e)))
        for lm in re.finditer(r"\bdo\s*\{", body):
            loops.append((lm.end() - 1, _match_close(body, lm.end() - 1, "{", "}")))
        for im in re.finditer(r"\bif\s*\(\s*!?\s*(\w+)\s*\)", body):
            if im.group(1) not in ptrs or not any(a <= im.start() < b for a, b in loops):
                continue
            t_end = _stmt_end(body, im.end())
            e = re.match(r"\s*else\b", body[t_end:])
            if e and _stores(body[im.end():t_end]) and _stores(body[t_end + e.end():_stmt_end(body, t_end + e.end())]):
                hits.append((m.group(1), im.group(1), line0 + body.count("\n", 0, im.start())))
    return hits


def test_no_kernel_picks_its_store_target_at_run_time_inside_a_loop():
    # the detector sees the form that failed ...
    bad = """
    __global__ void k_bad(const uint64_t *__restrict__ codes, uint32_t *bits, uint64_t *__restrict__ out_idx, int n) {
        for (;;) {
            if (out_idx) { for (int j = 0; j < n; ++j) out_idx[j] = codes[j]; }
            else { for (int j = 0; j < n; ++j) bit_set(bits, codes[j]); }
            if (n) break;
        }
    }"""
    assert run_time_store_target_choices(bad) == [("k_bad", "out_idx", 4)]
    # ... not an optional extra output, and not the choice made by a template parameter
    ok = """
    template <bool OUT> __global__ void k_ok(const uint64_t *__restrict__ codes, uint32_t *bits, uint64_t *__restrict__ out_idx, float *pos, int n) {
        for (int i = 0; i < n; ++i) {
            if (OUT) out_idx[i] = codes[i]; else bit_set(bits, codes[i]);
            if (pos) pos[i] = 1.0f;
        }
    }"""
    assert run_time_store_target_choices(ok) == []
    # One place is allowed, by name: k_cbf_heavy hands a run's final counters either to the filter or to the sharded engine's reply array ONCE per
    # run, after the loop that carries the run's state (rb_pipeline.hpp); both forms are compared with the oracle at sizes that fill the device
    # (tests/test_gpu_scale.py, tests/test_gpu_sharded.py scale tests, tools/parity_at_size.py).
    allowed = {("rb_pipeline.hpp", "k_cbf_heavy", "cfinal")}
    d = os.path.join(ROOT, "rna-bloom_amd", "csrc")
    found = set()
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".hpp")):
            for kern, ptr, line in run_time_store_target_choices(open(os.path.join(d, f)).read()):
                found.add((f, kern, ptr))
    assert found <= allowed, "run-time choice between store targets inside a kernel loop (make it a template parameter): %s" % sorted(found - allowed)


def test_library_carries_the_id_of_the_sources_it_was_built_from():
    """rb_build_id() == tools/csrc_id.py of the tree: what bench.py compares with the id stored beside the committed PMC summaries.  A stale
    library (built before the last source edit) FAILS here with the command that rebuilds it — a test does not rewrite the library other tests
    of the session have mapped."""
    import subprocess, sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import csrc_id
    want = csrc_id.csrc_id(ROOT)
    ask = [sys.executable, "-c", "import sys; sys.path[:0] = [%r]; from rnabloom import _native as N; print(N.lib.rb_build_id().decode())" % os.path.join(ROOT, "rna-bloom_amd")]
    got = subprocess.run(ask, capture_output=True, text=True, timeout=300).stdout.strip().splitlines()[-1:]
    assert got == [want], "librb_hip.so is stale (built from sources %s, the tree is %s): rebuild with `python -c 'import __graft_entry__ as g; g.build()'`" % (got, want)


# ---- the fault behind the round-1 "k_pairs_insert miscompile", found in round 5 (profiles/r05_miscompile.md, tools/microbench/shift_last): on gfx950 a 64-bit
#      shift (v_lshlrev_b64 / v_lshrrev_b64 / v_ashrrev_i64) whose 32-bit shift-amount operand is the LAST vector register the wavefront was allocated gives
#      wrong results now and then.  The compiler is free to produce that (it did, in one kernel of round 2), so every kernel of the library is checked. ----
def test_no_64_bit_shift_takes_its_amount_from_the_last_allocated_vgpr():
    """the scan itself lives in tools/check_shift_last.py: __graft_entry__.build() runs it on every build (a different hipcc point release on the
    driver's box cannot reintroduce the shape unseen), this test runs it on the library the session loaded"""
    import sys
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("no llvm-objdump")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_shift_last
    bad, kernels, shifts = check_shift_last.check_library(os.path.join(ROOT, "rna-bloom_amd", "lib", "librb_hip.so"))
    assert kernels > 100 and shifts > 100, (kernels, shifts)           # the scan saw the library (shifts whose amount is a vector register)
    assert not bad, "64-bit shifts with the shift amount in the wavefront's last VGPR (profiles/r05_miscompile.md): %s" % bad[:5]
