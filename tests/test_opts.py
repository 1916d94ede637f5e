"""sw_opts (include/sw_amd.h): the kernel-form overrides behind the C ABI.
CPU-only: no handle is created (sw_set_opts is checked for its argument
errors only; the GPU tests drive every field through the `knobs` fixture)."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "ece1782-smith-waterman-cuda_amd", "csrc")

ENV = {"lpt": "SW_LPT", "lpt_pipe": "SW_LPT_PIPE", "quad_width": "SW_QUAD_WIDTH", "pair_width": "SW_PAIR_WIDTH",
       "pair_group": "SW_PAIR_GROUP", "coop_width": "SW_COOP_WIDTH", "coop_skew": "SW_COOP_SKEW",
       "intra_x2": "SW_INTRA_X2", "intra_x2_rows": "SW_INTRA_X2_RI", "intra_i16_first": "SW_INTRA_I16_FIRST",
       "inter_i16_span": "SW_INTER_I16_SPAN", "int16_guard": "SW_INT16_GUARD", "rescue_stats": "SW_RESCUE_STATS",
       "tail_pairs": "SW_TAIL_PAIRS", "lpt_persist": "SW_LPT_PERSIST",
       "lpt_rows": "SW_LPT_ROWS", "tri_width": "SW_TRI_WIDTH",
       "lpt_pipe_tail": "SW_LPT_PIPE_TAIL", "drain_spin": "SW_DRAIN_SPIN"}


def test_init_is_all_auto_and_sized(sw):
    o = sw.capi.Opts()
    assert sw.capi.lib().sw_opts_init(ctypes.byref(o)) == 0
    assert o.size == ctypes.sizeof(sw.capi.Opts)  # the binding's layout is the header's
    d = o.as_dict()
    assert all(d[f] == -1 for f in sw.capi.Opts.INT_FIELDS)
    assert d["inter_variant"] == "" and d["trace_file"] == ""
    assert set(ENV) == set(sw.capi.Opts.INT_FIELDS)


def test_from_env_reads_each_variable(sw, monkeypatch):
    for f in ENV.values():
        monkeypatch.delenv(f, raising=False)
    assert all(v == -1 for k, v in sw.capi.opts_from_env().as_dict().items() if k in ENV)
    for k, (f, name) in enumerate(ENV.items()):
        monkeypatch.setenv(name, str(k + 3))
    monkeypatch.setenv("SW_INTER_VARIANT", "f32x4")
    monkeypatch.setenv("SW_TRACE_FILE", "/tmp/t.bin")
    d = sw.capi.opts_from_env().as_dict()
    for k, f in enumerate(ENV):
        assert d[f] == k + 3, f
    assert d["inter_variant"] == "f32x4" and d["trace_file"] == "/tmp/t.bin"


def test_set_opts_argument_errors(sw):
    L = sw.capi.lib()
    o = sw.capi.Opts()
    L.sw_opts_init(ctypes.byref(o))
    assert L.sw_set_opts(None, ctypes.byref(o)) == -1
    assert L.sw_get_opts(None, ctypes.byref(o)) == -1
    assert L.sw_opts_init(None) == -1
    assert L.sw_db_reset_adaptive(None) == -1


def test_no_environment_read_on_the_scan_path():
    """The library reads SW_* variables only in sw_opts_from_env (VERDICT r04
    item 8): the scan path's choices come from the handle's sw_opts."""
    # every source in the directory but the programs that link the library (the
    # Makefile's HOSTOBJS: the CLI and the C++ drop-in pick their devices from
    # SW_DEVICE & co.)
    programs = re.search(r"^HOSTOBJS\s*:=\s*(.+)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert sorted(programs) == ["main", "sw_cli", "sw_tests", "swsolver"]
    sources = sorted(s for s in os.listdir(CSRC)
                     if s.endswith((".cpp", ".hip", ".h")) and s.rsplit(".", 1)[0] not in programs)
    assert len(sources) >= 30 and "sw_hits.hip" in sources and "sw_plan.cpp" in sources
    defined_in = []
    for src in sources:
        text = open(os.path.join(CSRC, src)).read()
        calls = [m.start() for m in re.finditer(r"\bgetenv\(", text)]
        if "int sw_opts_from_env(" not in text:
            assert not calls, src
            continue
        defined_in.append(src)
        body = text[text.index("int sw_opts_from_env("):]
        body = body[:body.index("\n}\n")]
        start = text.index(body)
        assert calls and all(start <= c < start + len(body) for c in calls), "getenv outside sw_opts_from_env"
    assert len(defined_in) == 1, defined_in


def test_hip_resources_are_created_and_released_in_sw_host_h():
    """Every HIP resource of the host driver is held by an owner (DESIGN.md,
    "Who owns a HIP resource"): the calls that create or release device
    memory, pinned memory, events and streams occur in csrc/sw_host.h, behind
    the owners' helpers, and in no .cpp file, so no member or local can be
    released by hand, twice, or not at all."""
    # (by name, so a function passed as a release argument counts as well as a call)
    calls = re.compile(r"\b(hipFree|hipHostFree|hipEventDestroy|hipStreamDestroy|hipMalloc|hipHostMalloc)\b"
                       r"|\b(hipEventCreate|hipStreamCreate)")
    for src in sorted(os.listdir(CSRC)):
        if src.endswith(".cpp"):
            found = [m.group(0) for m in calls.finditer(open(os.path.join(CSRC, src)).read())]
            assert not found, (src, found)
    found = {m.group(1) or m.group(2) for m in calls.finditer(open(os.path.join(CSRC, "sw_host.h")).read())}
    assert found == {"hipFree", "hipHostFree", "hipEventDestroy", "hipStreamDestroy", "hipMalloc", "hipHostMalloc",
                     "hipEventCreate", "hipStreamCreate"}, found
