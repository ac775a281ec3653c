"""Every PRF kernel adds the replay's iter shift by hand: kernel arguments are frozen into a captured graph, and a replay becomes
another round only because each kernel adds the device word te0[kIterShiftWord] (device_common.h) to the iter it was launched with.  A
kernel that forgets still writes plausible ciphertexts -- with the previous round's mask streams.  tests/test_gpu_graph_replay.py
replays the kernels on the chip; this guard reads the sources, so that a NEW PRF kernel without the shift fails without a GPU.

A PRF kernel is a __global__ function of flashe_amd/csrc/*.hip whose parameter list starts with `const RoundKeys`, or that takes a
te0 table pointer.  Its text is its own body (braces matched, which is narrower than "up to the next __global__": a helper defined
behind it cannot vouch for it) with the .inc files the body includes."""
import glob
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flashe_amd", "csrc")
# aes_blocks_kernel: the known-answer test of the block cipher (flashe_selftest) -- it encrypts the blocks it is given and has no iter.
ALLOWED = {"aes_blocks_kernel"}
# tuning builds only (#ifdef FLASHE_TUNING): kernels a shipped library does not contain; none needs an exemption today
ALLOWED_UNDER_TUNING = set()
WORD = "kIterShiftWord"


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _matching(text, start, open_ch, close_ch):
    """Index just past the bracket that closes the one at text[start]."""
    depth = 0
    for i in range(start, len(text)):
        if text[i] == open_ch:
            depth += 1
        elif text[i] == close_ch:
            depth -= 1
            if depth == 0:
                return i + 1
    raise AssertionError("unbalanced %s at offset %d" % (open_ch, start))


def _kernels(text):
    """(name, parameter list, body with its .inc files) of every __global__ function DEFINED in `text` (comments stripped)."""
    out = []
    for m in re.finditer(r"__global__", text):
        head = re.match(r"\s*(?:__launch_bounds__\s*\([^()]*\)\s*)?(?:static\s+)?void\s+(\w+)\s*\(", text[m.end():])
        assert head, "a __global__ this scan cannot read: %r" % text[m.start():m.start() + 120]
        name, paren = head.group(1), m.end() + head.end() - 1
        end_params = _matching(text, paren, "(", ")")
        params = text[paren + 1:end_params - 1]
        rest = text[end_params:].lstrip()
        if not rest.startswith("{"):
            continue                                                            # a declaration
        brace = text.index("{", end_params)
        body = text[brace:_matching(text, brace, "{", "}")]
        for inc in re.findall(r'#include\s+"([^"]+\.inc)"', body):
            with open(os.path.join(CSRC, inc)) as f:
                body += "\n" + _strip_comments(f.read())
        out.append((name, params, body))
    return out


def _prf_kernels(text):
    # (the table pointer may travel inside a parameter struct -- the bit-sliced kernels take no RoundKeys, their te0 is PrfParams')
    carriers = "|".join(sorted(_structs_with_te0()))
    return [(n, b) for n, p, b in _kernels(_strip_comments(text))
            if re.match(r"\s*const\s+RoundKeys\b", p) or re.search(r"\bte0\b", p) or re.search(r"\b(%s)\b" % carriers, p)]


def _structs_with_te0():
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")):
        with open(path) as f:
            text = _strip_comments(f.read())
        for m in re.finditer(r"\bstruct\s+(\w+)\s*\{", text):
            if re.search(r"\bte0\s*;", text[m.end() - 1:_matching(text, m.end() - 1, "{", "}")]):
                names.add(m.group(1))
    assert "PrfParams" in names and "SmallParams" in names, names
    return names


def _all_sources():
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        with open(path) as f:
            yield os.path.basename(path), f.read()


def test_every_prf_kernel_adds_the_iter_shift():
    seen, missing = [], []
    for fname, text in _all_sources():
        for name, body in _prf_kernels(text):
            seen.append(name)
            if WORD not in body and name not in ALLOWED | ALLOWED_UNDER_TUNING:
                missing.append("%s:%s" % (fname, name))
    assert not missing, "PRF kernels that never read te0[%s] (a graph replay would reuse the captured round's masks): %s" % (WORD, missing)
    # the scan sees the kernels it is there for: the ones the issue names, and about twenty in all
    for name in ("prf_wide_kernel", "prf_small_kernel", "prf_wide_batch_kernel", "prf_small_jobs_kernel", "prf_chain_kernel", "prf_dec_sum128_kernel",
                 "prf_small_chain_kernel", "reduce_decrypt_ptrs_kernel", "small_reduce_decrypt_kernel", "small_reduce_decrypt_split_kernel",
                 "span_prf_kernel", "span_prf_small_kernel", "sparse_edge_prf_kernel", "aes_blocks_kernel"):
        assert name in seen, name
    assert len(seen) >= 20, seen
    # an exemption names a kernel that exists and that really has no shift
    for name in ALLOWED | ALLOWED_UNDER_TUNING:
        assert name in seen, name


def test_the_allowed_kernel_takes_no_iter():
    for _, text in _all_sources():
        for name, params, body in _kernels(_strip_comments(text)):
            if name in ALLOWED:
                assert not re.search(r"\biter\w*\b", params) and WORD not in body, name


@pytest.mark.parametrize("line", ["    const uint32_t iter = iter0 + te0[kIterShiftWord];", "    const uint32_t iter = p.iter + p.te0[kIterShiftWord];"])
def test_the_guard_sees_a_deleted_shift(line):
    """The scan run on sources with the shift deleted from one kernel (or one .inc body) at a time: each deletion is reported."""
    hits = 0
    for fname, text in _all_sources():
        for m in re.finditer(re.escape(line), text):
            cut = text[:m.start()] + line.replace(" + te0[kIterShiftWord]", "").replace(" + p.te0[kIterShiftWord]", "") + text[m.end():]
            before = {n for n, b in _prf_kernels(text) if WORD not in b}
            after = {n for n, b in _prf_kernels(cut) if WORD not in b}
            assert len(after - before) == 1, (fname, text.count("\n", 0, m.start()) + 1)
            hits += 1
    assert hits >= 3
