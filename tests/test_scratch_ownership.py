"""CPU check of who owns device memory inside the HIP back-end (bcnn_amd/csrc). Library-private device scratch has one
owner: the per-thread, per-device slot table of runtime.hip (common.h: ScratchSlot, scratch()). Besides it only the C-ABI
allocation entry points, the runtime warm-up, the prepack store of conv.hip and the window scheduler counters of
conv_window.hip call hipMalloc / hipFree, so that a kernel family cannot grow a grow-only allocator of its own again.
The pinned host side of the staged batches has one owner as well: the staging table of runtime.hip (common.h: StageSlot,
host_stage(), host_stage_extend(), stage_upload()); nothing else allocates pinned memory or records the event behind a
staging copy."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bcnn_amd", "csrc")

# file -> the functions in it that may allocate or free device memory
ALLOWED = {
    "runtime.hip": {"scratch", "warm_device_keeping_rand_state", "bcnn_hip_malloc_f32", "bcnn_hip_malloc_i32",
                    "bcnn_hip_free"},
    "conv.hip": {"prepack_free_all", "prepack_entry", "prepack_table"},
    "conv_window.hip": {"window_sched_slot"},
}
_TOKEN = re.compile(r'"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'|//[^\n]*|/\*.*?\*/', re.S)
_CALL = re.compile(r"\b(\w+)\s*\(")
_NOT_A_NAME = {"__launch_bounds__", "__attribute__", "alignas", "__declspec"}


def _strip_comments(text):
    """comments blanked out (newlines kept, so line numbers stay), string and character literals kept"""
    def repl(m):
        tok = m.group(0)
        return tok if tok[0] in "\"'" else re.sub(r"[^\n]", " ", tok)
    return _TOKEN.sub(repl, text)


def _sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(paths) > 30, paths
    return {os.path.basename(p): _strip_comments(open(p).read()) for p in paths}


def _enclosing_function(lines, i):
    """name of the function whose definition starts at the last column-0 line with a call-like token before line i"""
    for line in reversed(lines[:i]):
        if not line or line[0] in " \t#}":
            continue
        names = [n for n in _CALL.findall(line) if n not in _NOT_A_NAME]
        if names:
            return names[0]
    return None


def test_device_memory_is_allocated_only_by_its_owners():
    found = set()
    for fn, text in _sources().items():
        lines = text.split("\n")
        for i, line in enumerate(lines):
            if not re.search(r"\bhip(Malloc|Free)\w*\s*\(", line):
                continue
            owner = _enclosing_function(lines, i)
            assert owner in ALLOWED.get(fn, ()), \
                "%s:%d: device memory allocated or freed in %s(); library scratch belongs in the slot table of runtime.hip " \
                "(common.h: ScratchSlot)" % (fn, i + 1, owner)
            found.add((fn, owner))
    assert ("runtime.hip", "scratch") in found


def test_scratch_entry_points_are_declared_once_and_defined_once():
    src = _sources()
    decl = re.compile(r"^\s*(?:inline\s+)?float4?\s*\*\s*(scratch|scratch_f4)\s*\(\s*ScratchSlot\b[^)]*\)\s*([;{])", re.M)
    seen = {}
    for fn, text in src.items():
        for m in decl.finditer(text):
            seen.setdefault(m.group(1), []).append((fn, m.group(2)))
    assert sorted(seen.get("scratch", [])) == [("common.h", ";"), ("runtime.hip", "{")], seen
    assert seen.get("scratch_f4") == [("common.h", "{")], seen
    assert len(re.findall(r"\benum\s+ScratchSlot\b", "".join(src.values()))) == 1


# ---- the pinned host side: the per-thread, per-device staging table of runtime.hip (common.h: StageSlot) -------------------------
PINNED_OWNERS = {"host_stage", "host_stage_extend"}


def test_pinned_host_memory_is_allocated_only_by_the_staging_table():
    found = set()
    for fn, text in _sources().items():
        lines = text.split("\n")
        for i, line in enumerate(lines):
            if not re.search(r"\bhipHost(Malloc|Free|Alloc)\b", line):
                continue
            owner = _enclosing_function(lines, i)
            assert fn == "runtime.hip" and owner in PINNED_OWNERS, \
                "%s:%d: pinned host memory allocated or freed in %s(); staging blocks belong in the table of runtime.hip " \
                "(common.h: StageSlot)" % (fn, i + 1, owner)
            found.add(owner)
    assert found == PINNED_OWNERS


def test_staging_entry_points_are_declared_once_and_defined_once():
    src = _sources()
    decl = re.compile(r"^\s*uint8_t\s*\*\s*(host_stage|host_stage_extend|stage_upload)\s*\(\s*StageSlot\b[^)]*\)\s*([;{])", re.M)
    seen = {}
    for fn, text in src.items():
        for m in decl.finditer(text):
            seen.setdefault(m.group(1), []).append((fn, m.group(2)))
    for name in ("host_stage", "host_stage_extend", "stage_upload"):
        assert sorted(seen.get(name, [])) == [("common.h", ";"), ("runtime.hip", "{")], (name, seen)
        # and nothing of that name with another signature anywhere: every other mention is a call
        defs = [(fn, m.group(0)) for fn, text in src.items()
                for m in re.finditer(r"^[A-Za-z_][\w \*]*\b%s\s*\([^;{]*\)\s*[;{]" % name, text, re.M)]
        assert len(defs) == 2, (name, defs)
    assert len(re.findall(r"\benum\s+StageSlot\b", "".join(src.values()))) == 1


def test_the_copy_in_flight_is_recorded_only_by_the_staging_table():
    for fn, text in _sources().items():
        if fn == "runtime.hip":
            assert len(re.findall(r"\bhipEventRecord\s*\(\s*[\w.\->]*\bcopied\b", text)) == 1     # stage_upload
            continue
        for m in re.finditer(r"\bhipEventRecord\s*\(\s*[^,;]*\bcopied\b", text):
            raise AssertionError("%s: %s: the event behind a staging copy belongs to stage_upload (runtime.hip)"
                                 % (fn, m.group(0)))
