"""Build libmoira_pb.so (the HIP library behind the C ABI) in-tree with hipcc for gfx950.

    python -m moira_amd.build          # builds moira_amd/libmoira_pb.so if stale
    python -m moira_amd.build --force

hipcc cross-compiles gfx950 code objects without a GPU, so this runs in the build
container; the .so travels to the GPU box with the source snapshot.
-ffp-contract=off is REQUIRED: the DP cell and the interpolation must round exactly as the
reference (gcc, baseline x86-64, no FMA) does.
"""
import fcntl
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmoira_pb.so")
# the host side of the library: the C ABI layer, unit by unit (mpb_hostonly.cpp includes no HIP header), and the broker
HOST_SOURCES = [os.path.join(CSRC, name) for name in ("mpb_hostonly.cpp", "mpb_context.cpp", "mpb_resident.cpp", "mpb_hostfed.cpp",
                                                      "mpb_perread.cpp", "mpb_poisson.cpp", "mpb_text.cpp", "mpb_contig.cpp",
                                                      "mpb_bgzf.cpp", "mpb_inflate.cpp", "mpb_index.cpp", "mpb_bgzf_fastq.cpp",
                                                      "mpb_format.cpp", "mpb_collapse.cpp", "mpb_fasta_qual.cpp", "mpb_broker.cpp")]
CONTIG_KERNELS = os.path.join(CSRC, "mpb_contig_kernels.hip")      # k_contig: a kernel unit of its own (mpb_kernels.hip stays as it is)
BGZF_KERNELS = os.path.join(CSRC, "mpb_bgzf_kernels.hip")          # k_bgzf_deflate / _scan / _frame: .gz output, a unit of its own as well
INFLATE_KERNELS = os.path.join(CSRC, "mpb_inflate_kernels.hip")    # k_bgzf_inflate: BGZF .gz input, one more unit of its own
INDEX_KERNELS = os.path.join(CSRC, "mpb_index_kernels.hip")        # k_fq_lines / _scan / _starts / _rows: the FASTQ record index, likewise
CRC_KERNELS = os.path.join(CSRC, "mpb_crc_kernels.hip")            # k_bgzf_crc32: the CRC-32 of inflated text where it lies, likewise
PAIR_KERNELS = os.path.join(CSRC, "mpb_pair_kernels.hip")          # k_pair_rows / _count / _scan / _lists: two record indexes -> k_contig's inputs, likewise
FORMAT_KERNELS = os.path.join(CSRC, "mpb_format_kernels.hip")      # k_fmt_count / _scan / _write: output records from text + index, likewise
COLLAPSE_KERNELS = os.path.join(CSRC, "mpb_collapse_kernels.hip")  # k_col_hash / _group / _rep: hashes and first equal records of a chunk, likewise
FASTA_QUAL_KERNELS = os.path.join(CSRC, "mpb_fasta_qual_kernels.hip")  # k_fa_count / _scan / _write: fasta + qual text -> slots and index, likewise
SOURCES = [os.path.join(CSRC, "mpb_kernels.hip"), CONTIG_KERNELS, BGZF_KERNELS, INFLATE_KERNELS, INDEX_KERNELS, CRC_KERNELS,
           PAIR_KERNELS, FORMAT_KERNELS, COLLAPSE_KERNELS, FASTA_QUAL_KERNELS] + HOST_SOURCES
DEPS = SOURCES + [os.path.join(CSRC, "mpb_internal.h"), os.path.join(CSRC, "mpb_host_internal.h"),
                  os.path.join(CSRC, "mpb_shared.h"), os.path.join(CSRC, "mpb_hostonly.h"), os.path.join(CSRC, "mpb_ctx.h"),
                  os.path.join(CSRC, "mpb_queue.h"),
                  os.path.join(CSRC, "mpb_dp_tiles.inc"),
                  os.path.join(CSRC, "mpb_narrow_ring.inc"), os.path.join(CSRC, "mpb_narrow_rs.inc"),
                  os.path.join(CSRC, "mpb_narrow_rg.inc"),
                  os.path.join(CSRC, "mpb_contig_lane.inc"), os.path.join(CSRC, "mpb_contig_args.h"),
                  os.path.join(CSRC, "mpb_contig_rows.inc"),
                  os.path.join(CSRC, "mpb_bgzf_lane.inc"),
                  os.path.join(CSRC, "mpb_inflate_lane.inc"),
                  os.path.join(CSRC, "mpb_index_lane.inc"),
                  os.path.join(CSRC, "mpb_crc_lane.inc"),
                  os.path.join(CSRC, "mpb_pair_lane.inc"),
                  os.path.join(CSRC, "mpb_format_lane.inc"),
                  os.path.join(CSRC, "mpb_collapse_lane.inc"),
                  os.path.join(CSRC, "mpb_fasta_qual_lane.inc"),
                  os.path.join(CSRC, "contig_posterior.h"),
                  os.path.join(CSRC, "libmoira_pb.map"),
                  os.path.join(ROOT, "include", "moira_pb.h"),
                  os.path.join(ROOT, "include", "mpb_synth.h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-shared", "-std=c++17",
         "-ffp-contract=off", "-fno-fast-math", "-pthread", "-Wall", "-Wno-unused-function",
         # a kernel that misses its occupancy target (k_dp at 2 waves per SIMD because a new caller of the shared class bodies
         # allowed them more registers) must fail the build, not cost 40 % silently
         "-Werror=pass-failed",
         "-fvisibility=hidden",          # only what include/moira_pb.h declares is exported ...
         "-Wl,--version-script=" + os.path.join(CSRC, "libmoira_pb.map"),   # ... not even weak std:: template instances
         "-x", "hip"]


CONTIG_LIB = os.path.join(HERE, "libmoira_contig.so")
CONTIG_SRC = os.path.join(CSRC, "contig.cpp")
CXX = os.environ.get("CXX", "g++")


CONTIG_DEPS = [CONTIG_SRC, os.path.join(CSRC, "contig_posterior.h"), os.path.join(ROOT, "include", "moira_contig.h"),
               os.path.join(ROOT, "include", "moira_io.h")]


def _digest(paths, flags):
    h = hashlib.sha256(" ".join(flags).encode())
    for p in paths:
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def _is_stale(lib, deps, flags):
    """A library is current when the digest of its sources + flags matches the stamp written next to it
    (file times do not survive the copy to a GPU box)."""
    stamp = lib + ".stamp"
    if not os.path.exists(lib) or not os.path.exists(stamp):
        return True
    try:
        return open(stamp).read().strip() != _digest(deps, flags)
    except OSError:
        return True


def _locked_build(lib, deps, flags, cmd, force, verbose):
    """Build under an exclusive lock: the ranks of a multi-GPU job import the package at the same time."""
    with open(lib + ".lock", "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        try:
            if force or _is_stale(lib, deps, flags):
                if verbose:
                    print(" ".join(cmd))
                tmp = lib + ".tmp.%d" % os.getpid()
                subprocess.check_call(cmd[:-1] + [tmp])
                os.replace(tmp, lib)
                with open(lib + ".stamp", "w") as f:
                    f.write(_digest(deps, flags))
                if verbose:
                    print("%s: COMPILED now (sources + flags digest %s)" % (os.path.basename(lib), _digest(deps, flags)[:16]))
            elif verbose:
                print("%s: up to date" % os.path.basename(lib))
        finally:
            fcntl.flock(lk, fcntl.LOCK_UN)
    return lib


def report(lib, deps, flags):
    """One line saying what build() found: VERDICT r3 asked that a no-op build be visible as such."""
    state = "STALE" if _is_stale(lib, deps, flags) else "up to date: its stamp equals the digest of its sources + flags"
    print("%s: %s (digest %s, %d bytes)" % (os.path.basename(lib), state, _digest(deps, flags)[:16],
                                            os.path.getsize(lib) if os.path.exists(lib) else 0))


CONTIG_FLAGS = ["-O3", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-pthread", "-Wall"]


def contig_stale():
    return _is_stale(CONTIG_LIB, CONTIG_DEPS, CONTIG_FLAGS)


def build_contig(force=False, verbose=False):
    """CPU-only contig construction library (g++, no HIP): north_star keeps NW on the CPU."""
    if not force and not contig_stale():
        return CONTIG_LIB
    cmd = [CXX] + CONTIG_FLAGS + [CONTIG_SRC, "-o", CONTIG_LIB]
    return _locked_build(CONTIG_LIB, CONTIG_DEPS, CONTIG_FLAGS, cmd, force, verbose)


IO_LIB = os.path.join(HERE, "libmoira_io.so")
IO_SRC = os.path.join(CSRC, "fastio.cpp")
IO_SRC2 = os.path.join(CSRC, "inflate.cpp")
IO_DEPS = [IO_SRC, IO_SRC2, os.path.join(ROOT, "include", "moira_io.h")]
IO_FLAGS = ["-O3", "-fPIC", "-shared", "-std=c++17", "-pthread", "-Wall"]


def io_stale():
    return _is_stale(IO_LIB, IO_DEPS, IO_FLAGS)


def build_io(force=False, verbose=False):
    """CPU-only text I/O library of the CLI (g++, no HIP): FASTQ indexing, packing, record formatting."""
    if not force and not io_stale():
        return IO_LIB
    cmd = [CXX] + IO_FLAGS + [IO_SRC, IO_SRC2, "-o", IO_LIB]
    return _locked_build(IO_LIB, IO_DEPS, IO_FLAGS, cmd, force, verbose)


def stale():
    return _is_stale(LIB, DEPS, FLAGS)


def build(force=False, verbose=False, extra=()):
    if not force and not stale() and not extra:
        return LIB
    cmd = [HIPCC] + FLAGS + list(extra) + SOURCES + ["-o", LIB]
    return _locked_build(LIB, DEPS, FLAGS + list(extra), cmd, force or bool(extra), verbose)


if __name__ == "__main__":
    if "--host-sources" in sys.argv:     # for scripts that build variants of the library (tools/experiments)
        print(" ".join(os.path.relpath(p, ROOT) for p in HOST_SOURCES))
        sys.exit(0)
    if "--units-beside-kernels" in sys.argv:     # every unit besides mpb_kernels.hip, which such a script replaces by its variant
        print(" ".join(os.path.relpath(p, ROOT) for p in [CONTIG_KERNELS, BGZF_KERNELS, INFLATE_KERNELS, INDEX_KERNELS, CRC_KERNELS, PAIR_KERNELS, FORMAT_KERNELS, COLLAPSE_KERNELS, FASTA_QUAL_KERNELS] + HOST_SOURCES))
        sys.exit(0)
    build(force="--force" in sys.argv, verbose=True)
    build_contig(force="--force" in sys.argv, verbose=True)
    build_io(force="--force" in sys.argv, verbose=True)
    print(LIB)
    print(CONTIG_LIB)
    print(IO_LIB)
