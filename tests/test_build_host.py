"""photonbend_amd/build.py and tests/kernel_listing.py without a compiler or a GPU: every hipcc command line the build can produce (the literals
were recorded from the build functions and the listing script as they were before the build got one description of its compiles), the one
staleness rule, the host's math flavour, the one compile the six test_isa_*.py modules share, and the listing reader against a cut of a
real listing (tests/golden/listing_excerpt.txt: three kernels of the product build, each from its label through its Occupancy line)."""

import os
import shutil
import types

import pytest

from photonbend_amd import build
from tests import helpers as H
from tests import kernel_listing

EXCERPT = os.path.join(H.GOLD, "listing_excerpt.txt")


@pytest.fixture
def recorded(monkeypatch, tmp_path):
    """hipcc found at a fixed place, every compile replaced by a recorder that succeeds, the diagnostic library in a build/ that is not there yet"""
    argvs = []

    def run(cmd, **kw):
        argvs.append(list(cmd))
        return types.SimpleNamespace(returncode=0, stdout="", stderr="")

    monkeypatch.setattr(build, "subprocess", types.SimpleNamespace(run=run))
    monkeypatch.setattr(build, "hipcc", lambda: "/somewhere/hipcc")
    monkeypatch.setattr(build, "DIAG_LIB_PATH", str(tmp_path / "build" / "libphotonbend_hip_diag.so"))
    return argvs


def test_every_hipcc_command_line_is_the_one_it_was(recorded, monkeypatch, tmp_path):
    src = os.path.join(build.CSRC, "photonbend_hip.hip")
    library = ["/somewhere/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-mllvm", "-disable-machine-licm", "-fPIC", "-shared",
               "-fvisibility=hidden", "-Wall", "-Wno-unused-function"]
    listing = ["/somewhere/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-mllvm", "-disable-machine-licm", "-Wall",
               "-Wno-unused-function"]
    other, s = str(tmp_path / "other.so"), str(tmp_path / "pb.s")

    monkeypatch.setenv("PB_MATH_FLAVOUR", "svml")
    assert build.variants() == {"product": (build.LIB_PATH, ()), "libm": (build.LIBM_LIB_PATH, ("PB_MATH_LIBM",)),
                                "diagnostic": (build.DIAG_LIB_PATH, ("PB_ABLATION",))}
    assert build.build_library(force=True) == build.LIB_PATH
    assert build.build_libm_flavour(force=True) == build.LIBM_LIB_PATH
    assert not os.path.exists(os.path.dirname(build.DIAG_LIB_PATH))
    assert build.build_diagnostic(force=True) == build.DIAG_LIB_PATH
    assert os.path.isdir(os.path.dirname(build.DIAG_LIB_PATH))  # (build/ is made where it is missing)
    monkeypatch.setenv("PB_MATH_FLAVOUR", "libm")
    assert build.build_diagnostic(force=True) == build.DIAG_LIB_PATH
    assert build.build_library(out=other, defines=("PB_STAMPS",)) == other  # (another path: always compiled)
    assert build.build_listing(s) == s
    assert build.build_listing(s, defines=("PB_ABLATION",)) == s
    assert recorded == [
        library + [src, "-o", build.LIB_PATH],
        library + ["-DPB_MATH_LIBM", src, "-o", build.LIBM_LIB_PATH],
        library + ["-DPB_ABLATION", src, "-o", build.DIAG_LIB_PATH],
        library + ["-DPB_ABLATION", "-DPB_MATH_LIBM", src, "-o", build.DIAG_LIB_PATH],
        library + ["-DPB_STAMPS", src, "-o", other],
        listing + ["-S", "--cuda-device-only", "-o", s, src],
        listing + ["-DPB_ABLATION", "-S", "--cuda-device-only", "-o", s, src],
    ]


def test_an_up_to_date_library_is_not_compiled_again(recorded, monkeypatch):
    monkeypatch.setattr(build, "stale", lambda path: False)
    assert (build.build_library(), build.build_libm_flavour(), build.build_diagnostic()) == (build.LIB_PATH, build.LIBM_LIB_PATH, build.DIAG_LIB_PATH)
    assert recorded == []
    monkeypatch.setattr(build, "stale", lambda path: True)
    build.build_library(), build.build_libm_flavour(), build.build_diagnostic()
    assert [a[-1] for a in recorded] == [build.LIB_PATH, build.LIBM_LIB_PATH, build.DIAG_LIB_PATH]


def test_a_failed_compile_raises_with_the_compilers_words(monkeypatch, tmp_path):
    failed = types.SimpleNamespace(returncode=1, stdout="", stderr="pb_kernels.hpp:7: error: no such thing")
    monkeypatch.setattr(build, "subprocess", types.SimpleNamespace(run=lambda cmd, **kw: failed))
    monkeypatch.setattr(build, "hipcc", lambda: "/somewhere/hipcc")
    for compile_ in (lambda: build.build_listing(str(tmp_path / "pb.s")), lambda: build.build_library(out=str(tmp_path / "x.so"))):
        with pytest.raises(RuntimeError, match="pb_kernels.hpp:7: error: no such thing"):
            compile_()


def test_stale(monkeypatch, tmp_path):
    csrc, header, target = tmp_path / "csrc", tmp_path / "photonbend_hip.h", tmp_path / "lib.so"
    csrc.mkdir()
    deps = [csrc / "a.hip", csrc / "b.hpp", header]
    for d in deps:
        d.write_text("")
        os.utime(d, (1000, 1000))
    monkeypatch.setattr(build, "CSRC", str(csrc))
    monkeypatch.setattr(build, "HEADER", str(header))
    assert build.stale(str(target))  # missing
    target.write_text("")
    os.utime(target, (2000, 2000))
    assert not build.stale(str(target))  # newer than everything
    os.utime(deps[1], (3000, 3000))
    assert build.stale(str(target))  # older than one source
    os.utime(deps[1], (1000, 1000))
    assert not build.stale(str(target))
    os.utime(header, (3000, 3000))
    assert build.stale(str(target))  # older than the header


def test_the_real_dependencies_are_the_sources_and_the_public_header():
    assert os.path.isdir(build.CSRC) and build.sources() == [os.path.join(build.CSRC, "photonbend_hip.hip")]
    assert build.HEADER == os.path.join(os.path.dirname(os.path.dirname(build.CSRC)), "include", "photonbend_hip.h") and os.path.isfile(build.HEADER)


def test_host_math_flavour(monkeypatch):
    from photonbend_amd import _native

    assert _native.host_math_flavour is build.host_math_flavour
    for value, want in (("svml", "svml"), ("libm", "libm"), ("LIBM", "libm"), ("SvMl", "svml")):
        monkeypatch.setenv("PB_MATH_FLAVOUR", value)
        assert build.host_math_flavour() == want
    monkeypatch.delenv("PB_MATH_FLAVOUR")
    hosts = build.host_math_flavour()
    assert hosts in ("svml", "libm")
    for value in ("", "avx512", "libm "):  # (not a flavour: the host's own)
        monkeypatch.setenv("PB_MATH_FLAVOUR", value)
        assert build.host_math_flavour() == hosts


# what the listing reader of the commit before it moved here returned for the excerpt (and, for these kernels, for the whole listing)
EXCERPT_ROWS = [
    {"mangled": "_Z21pb_store_words_kernel11PbWordChunkPii", "name": "pb_store_words_kernel", "vgpr": 2, "agpr": 0, "sgpr": 10, "scratch": 0,
     "occupancy": 8, "f64": 0, "valu": 2, "instr": 12, "lane_traffic": 0},
    {"mangled": "_Z20pb_save_flags_kernelPK11PbTileEntryPij", "name": "pb_save_flags_kernel", "vgpr": 4, "agpr": 0, "sgpr": 11, "scratch": 0,
     "occupancy": 8, "f64": 0, "valu": 6, "instr": 20, "lane_traffic": 0},
    {"mangled": "_Z22pb_gather_blend_kernelIhEvPKiPKdPKT_Phyi", "name": "pb_gather_blend_kernel<unsigned char>", "vgpr": 16, "agpr": 0, "sgpr": 22,
     "scratch": 0, "occupancy": 8, "f64": 7, "valu": 33, "instr": 77, "lane_traffic": 0},
]


def test_parse_reads_the_excerpt_as_it_always_did():
    if not shutil.which("c++filt"):
        pytest.skip("no c++filt")
    with open(EXCERPT) as f:
        assert kernel_listing.parse(f.read()) == EXCERPT_ROWS


def _counting_listing(monkeypatch, fails=False):
    calls = []

    def build_listing(out, defines=()):
        calls.append(out)
        if fails:
            raise RuntimeError("hipcc failed (1):\n\nerror: no such thing")
        shutil.copy(EXCERPT, out)
        return out

    monkeypatch.setattr(kernel_listing, "_stats", None)  # (and whatever this process has compiled comes back afterwards)
    monkeypatch.setattr(build, "build_listing", build_listing)
    monkeypatch.setattr(build, "hipcc", lambda: "/somewhere/hipcc")
    return calls


def test_stats_compiles_once(monkeypatch):
    if not shutil.which("c++filt"):
        pytest.skip("no c++filt")
    calls = _counting_listing(monkeypatch)
    first = kernel_listing.stats()
    assert kernel_listing.stats() is first and len(calls) == 1
    assert first == {r["name"]: r for r in EXCERPT_ROWS}
    assert not os.path.exists(os.path.dirname(calls[0]))  # (the listing does not stay behind)


def test_stats_remembers_a_failed_compile(monkeypatch):
    calls = _counting_listing(monkeypatch, fails=True)
    for _ in range(2):
        with pytest.raises(RuntimeError, match="error: no such thing"):
            kernel_listing.stats()
    assert len(calls) == 1


def test_stats_skips_without_hipcc(monkeypatch):
    calls = _counting_listing(monkeypatch)

    def no_hipcc():
        raise RuntimeError("hipcc not found")

    monkeypatch.setattr(build, "hipcc", no_hipcc)
    with pytest.raises(pytest.skip.Exception, match="needs hipcc"):
        kernel_listing.stats()
    assert calls == []
