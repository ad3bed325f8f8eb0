"""CPU: the two entry points of mixed-task training (merlin_env_set_difficulties, merlin_episode_class_stats) in the
header, the built library and the ctypes binding; the ABI version unchanged (they are additions)."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "merlin_hip.h")
NEW = ("merlin_env_set_difficulties", "merlin_episode_class_stats")


def test_header_declares_both_entry_points():
    src = open(HEADER).read()
    for s in NEW:
        assert re.search(r"^int " + s + r"\(", src, re.M), s
    # the signatures the issue sets
    flat = re.sub(r"\s+", " ", src)
    assert ("int merlin_env_set_difficulties(merlin_env *env, const int32_t *diff_host, int32_t n, void *stream);"
            in flat)
    assert ("int merlin_episode_class_stats(const float *done_dev, const double *ep_return_dev, "
            "const int32_t *ep_length_dev, const uint8_t *class_dev, int32_t T, int32_t N, int32_t n_classes, "
            "double *out_dev, int32_t accumulate, void *stream);" in flat)
    assert re.search(r"^#define MERLIN_ABI_VERSION 3\b", src, re.M)
    assert re.search(r"^#define MERLIN_ENV_CONFIG_FIELDS 10\b", src, re.M)


def test_library_exports_and_binding_lists_them():
    from merlin import _native as nat

    L = nat.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (merlin_\w+)", out))
    for s in NEW:
        assert s in exported, s
        assert s in nat.EXPORTED_SYMBOLS, s
        assert getattr(L, s).argtypes is not None, s
    assert len(L.merlin_env_set_difficulties.argtypes) == 4
    assert len(L.merlin_episode_class_stats.argtypes) == 10
    assert L.merlin_version() == nat.ABI_VERSION == 3


def test_host_side_refusals():
    """Argument checks that return before any device call."""
    from merlin import _native as nat

    L = nat.lib()
    assert L.merlin_env_set_difficulties(None, None, 0, None) == nat.E_INVALID
    assert L.merlin_episode_class_stats(None, None, None, None, 0, 0, 9, None, 0, None) == nat.E_INVALID
    assert b"n_classes" in L.merlin_last_error()
    assert L.merlin_episode_class_stats(None, None, None, None, -1, 4, 5, None, 0, None) == nat.E_INVALID
    assert L.merlin_episode_class_stats(None, None, None, None, 0, 0, 5, None, 0, None) == nat.E_INVALID  # no out


def test_integration_stub_agrees_with_the_binding():
    """INTEGRATION.md's ctypes stub lists both entry points with as many arguments as the header and the binding."""
    from merlin import _native as nat

    L = nat.lib()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    hdr = re.sub(r"\s+", " ", open(HEADER).read())
    for s in NEW:
        m = re.search(r"_L\." + s + r"\.argtypes = \[([^\]]*)\]", doc)
        assert m, s
        n_doc = len([a for a in m.group(1).split(",") if a.strip()])
        n_hdr = len(re.search(r"int " + s + r"\(([^)]*)\);", hdr).group(1).split(","))
        assert n_doc == n_hdr == len(getattr(L, s).argtypes), (s, n_doc, n_hdr)
