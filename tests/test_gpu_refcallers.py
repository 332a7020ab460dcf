"""The reference's own test programs, unchanged, on the HIP library (the caller-level drop-in,
SURVEY.md section 8(b): tests/contract.cpp:215-222, dist.cpp:253-259, bsr.cpp:759-766).

oracle/_ref/callers/* are superbblas's tests/{bsr,contract,dist,blas,dense}.cpp compiled against
include/superbblas.h and linked to libsuperbblas_amd.so (oracle/Makefile `callers`, built by
build() where the reference's sources are present).  Each runs its CPU-context section (host tensors mirrored
through the GPU) and its GPU sections; every section must print exactly the events the
reference itself prints for the same invocation (tests/golden/refcallers.json): the same
"Time in ..." steps, the same "Caught error: ..." lines -- including the reference's own known
failures (its Kronecker check at 12x12 blocks, bsr.cpp:860, and the invalid copy of its check
with --power=2) -- and "Everything went ok!" for contract.cpp's brute-force comparisons.
"""
import json
import os
import subprocess

import pytest

from _refcallers import INVOCATIONS, STORAGE_DETAILS, STORAGE_FILES, details_key, events, key

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "callers")
GOLDEN = json.load(open(os.path.join(HERE, "golden", "refcallers.json")))


def _run(name, args, env, cwd=None):
    exe = os.path.join(BIN, name)
    if not os.path.exists(exe):
        pytest.fail("%s missing: build it where the reference's sources are (make -C oracle callers)" % exe)
    e = dict(os.environ, OMP_NUM_THREADS="8", **env)
    e.pop("SB_TRACK_TIME", None)
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=e, timeout=240, cwd=cwd)
    assert r.returncode == 0, (name, args, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "libsuperbblas_amd" not in r.stderr, r.stderr[-2000:]
    return r.stdout


def _sections(ev):
    """events grouped by the section they were printed in (in order)"""
    out = []
    for sec, e in ev:
        if not out or out[-1][0] != sec:
            out.append((sec, []))
        out[-1][1].append(e)
    return [(s.split("|", 1)[1], e) for s, e in out]


@pytest.mark.parametrize("inv", [i for i in INVOCATIONS if i[0] in ("bsr", "dense")],
                         ids=lambda i: key(*i).replace(" ", "_"))
def test_sections_match_reference(gpu, inv):
    """bsr.cpp / dense.cpp: the CPU-context section and each GPU section (float and
    complex<double> for bsr) print the reference's CPU section's events"""
    name, args, env = inv
    ref = _sections([tuple(x) for x in GOLDEN[key(*inv)]])
    assert len(ref) == 1
    got = _sections(events(name, _run(name, args, env)))
    kinds = [s for s, _ in got]
    assert kinds[0].startswith(">>> CPU") and all(k.startswith(">>> GPU") for k in kinds[1:]), kinds
    assert len(got) == (3 if name == "bsr" else 2), kinds
    for sec, ev in got:
        assert ev == ref[0][1], (sec, ev, ref[0][1])


@pytest.mark.parametrize("inv", [i for i in INVOCATIONS if i[0] == "contract"],
                         ids=lambda i: key(*i).replace(" ", "_"))
def test_contract_cases(gpu, inv):
    """contract.cpp --test=N: case N of its exhaustive label-order / conj / alpha / beta /
    distribution sweep, in CPU and GPU contexts, against its brute-force contraction"""
    name, args, env = inv
    assert [e for _, e in GOLDEN[key(*inv)]] == ["Everything went ok!"]
    out = _run(name, args, env)
    assert [e for _, e in events(name, out)] == ["Everything went ok!"], out[-2000:]


def test_dist_program(gpu):
    """dist.cpp: distribution known answers, make_hole invariants, permuting copies into slices,
    shifts, the skinny and square GEMM shapes through detail::xgemm_batch_strided, the column- and
    row-major contractions, a GPU x CPU contraction, halo copies"""
    inv = [i for i in INVOCATIONS if i[0] == "dist"][0]
    ref = _sections([tuple(x) for x in GOLDEN[key(*inv)]])
    got = _sections(events(inv[0], _run(*inv)))
    assert [s for s, _ in got] == [">>> CPU tests:", ">>> GPU tests:"]
    assert got[0][1] == ref[0][1]
    extra = "Time in contracting xyz in column major (gpu x cpu -> gpu) #"
    assert [e for e in got[1][1] if e != extra] == ref[0][1] and extra in got[1][1]


def test_blas_program(gpu):
    """blas.cpp: detail::copy_n / copy_n_blocking with and without index vectors, scale factors,
    Copy and Add, all four scalar types, between host, pinned host and device memory, checked by
    the program against host loops (check_are_equal, 100 epsilon)"""
    inv = [i for i in INVOCATIONS if i[0] == "blas"][0]
    ref = _sections([tuple(x) for x in GOLDEN[key(*inv)]])
    got = _sections(events(inv[0], _run(*inv)))
    assert [s for s, _ in got] == [s for s, _ in ref] == ["- Non-blocking:", "- Blocking:"]
    # each section: the reference's CPU-context operations, then the same on the GPU context
    for (_, g), (_, r) in zip(got, ref):
        assert g == r + r


def test_contract_strided_sample(gpu):
    """contract.cpp's exhaustive sweep (1 327 104 cases: every T/A/B/C size, operand orders, conj,
    alpha / beta, distributions; double then complex<double>, CPU then GPU contexts,
    tests/contract.cpp:393-433, 475-500), sampled at a stride of 2111 across both scalar types
    (629 cases, 8 processes at a time; 1001 cases took 111 s on the GPU box).  The whole sweep, one process, passes in 6 min on the
    GPU box (profiles/r06_contract_full_sweep.txt)."""
    import concurrent.futures
    exe = os.path.join(BIN, "contract")
    if not os.path.exists(exe):
        pytest.fail("%s missing: build it where the reference's sources are (make -C oracle callers)" % exe)
    cases = list(range(11, 1327104, 2111))
    e = dict(os.environ, OMP_NUM_THREADS="2")
    e.pop("SB_TRACK_TIME", None)

    def one(t):
        r = subprocess.run([exe, "--test=%d" % t], capture_output=True, text=True, env=e, timeout=120)
        ok = r.returncode == 0 and "Everything went ok!" in r.stdout
        return t, ok, (r.stdout[-500:] + r.stderr[-500:]) if not ok else ""

    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        bad = [(t, msg) for t, ok, msg in pool.map(one, cases) if not ok]
    assert not bad, bad[:3]
    assert len(cases) == 629


def test_storage_program(gpu, tmp_path):
    """storage.cpp (the S3T tensor storage): create / append / read / check with no,
    per-block and global checksums, float and complex<double>, CPU contexts (mirrored through the
    GPU), then its GPU section (complex<double>, block checksums); every value read back is checked
    by the program (storage.cpp:280-351), as are the metadata, dimensions and type it recovers,
    and its checksum associativity test (do_checksum, storage.h:701-731).  The CPU sections print
    the reference's events, the GPU section those of the reference's block-checksum run."""
    inv = [i for i in INVOCATIONS if i[0] == "storage"][0]
    ref = _sections([tuple(x) for x in GOLDEN[key(*inv)]])
    got = _sections(events(inv[0], _run(*inv, cwd=str(tmp_path))))
    kinds = [k for k, _ in got]
    assert kinds == [k for k, _ in ref] + [">>> test for complex double"], kinds
    for (_, g), (_, r) in zip(got, ref):
        assert g == r
    # the GPU section: one block-checksum test (the reference's six events of that mode)
    assert got[-1][1] == ref[-1][1][6:12]


@pytest.mark.parametrize("fname", STORAGE_FILES)
@pytest.mark.parametrize("args", STORAGE_DETAILS, ids=lambda a: a[1])
def test_storage_details_program(gpu, fname, args):
    """storage_details.cpp (the reference's S3T inspection tool: read_storage_header, open_storage,
    check_storage, get_blocks) on the golden storage files the reference wrote: the same output as
    the reference's own build -- except the order of the listed blocks, which the reference takes
    from its block hash and this library from the append order (DESIGN, storage notes)"""
    exe = os.path.join(BIN, "storage_details")
    if not os.path.exists(exe):
        pytest.fail("%s missing: build it where the reference's sources are (make -C oracle callers)" % exe)
    r = subprocess.run([exe, os.path.join(HERE, "golden", fname)] + list(args), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    ref = GOLDEN[details_key(fname, args)]
    if "--list-blocks" in args:
        head_got, _, blocks_got = r.stdout.partition("blocks:\n")
        head_ref, _, blocks_ref = ref.partition("blocks:\n")
        assert head_got == head_ref
        assert sorted(blocks_got.splitlines()) == sorted(blocks_ref.splitlines())
    else:
        assert r.stdout == ref
