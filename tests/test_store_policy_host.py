"""CPU: the resident-buffer rule of the large single-asset observation store (finenvs_amd/csrc/fe_store_policy.h).

launch_env decides per launch whether the observation streams past the 256 MiB Infinity Cache (sc1 | nt, 1) or is stored
plain (sc1, 0).  The decision is a pure inline function of (what the env remembers, buffer pointer, buffer size) in a header
without HIP includes; this test compiles a few lines of host C++ around that header with the system compiler and drives it
with pointer sequences.  The expected strings are written out by hand from the rule:

  * size class 128 MiB <= bytes <= 256 MiB; below it never streams, above it always streams, neither touches the state;
  * the env remembers ONE resident buffer; a launch that writes it stores plain, a launch that writes any other streams;
  * when 8 consecutive launches have not written the resident buffer (at once when there is none yet), the buffer of that
    launch becomes the resident one for the launches after it -- the launch itself still streams.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(REPO, "finenvs_amd", "csrc")

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fe_store_policy.h"

// argv: tokens "<label><MiB>" (label = one letter, or '#' = a pointer never seen before); prints one policy digit per
// token, then the resident label and the away count.
int main(int argc, char **argv) {
    static char pool[26 + 4096];
    FeObsResidency st;
    int fresh = 0;
    for (int i = 1; i < argc; ++i) {
        const char lab = argv[i][0];
        const void *ptr = lab == '#' ? (const void *)&pool[26 + fresh++] : (const void *)&pool[lab - 'A'];
        const double mib = atof(argv[i] + 1);
        const uint64_t bytes = (uint64_t)(mib * 1048576.0);
        putchar('0' + fe_obs_store_policy(st, ptr, bytes));
    }
    const char *res = (const char *)st.resident.load();
    char name = '-';
    if (res) name = res >= pool + 26 ? '#' : (char)('A' + (res - pool));
    printf(" %c %d\n", name, st.away.load());
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "the system C++ compiler is needed to test the host-side store policy"
    d = tmp_path_factory.mktemp("store_policy")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    # no HIP include path, no hipcc: the header must stand on the standard library alone
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", HEADER_DIR, src, "-o", exe])

    def run(tokens, mib=160):
        toks = [t if any(ch.isdigit() for ch in t) else f"{t}{mib}" for t in tokens]
        out = subprocess.check_output([exe] + toks, text=True, timeout=60).split()
        return out[0], out[1], int(out[2])

    return run


def test_header_has_no_hip_include():
    s = open(os.path.join(HEADER_DIR, "fe_store_policy.h")).read()
    assert "hip" not in "".join(l for l in s.splitlines() if l.lstrip().startswith("#include"))


def test_one_buffer_is_absorbed_from_its_second_launch(driver):
    # config 2's observation is 160 MiB; the first launch adopts the buffer (and streams), every later one stores plain
    assert driver(list("A" * 12)) == ("1" + "0" * 11, "A", 0)


def test_ring_of_two_keeps_one_member_resident_and_streams_the_other(driver):
    pol, res, away = driver(list("AB" * 10))
    assert pol == "11" + "01" * 9
    assert (res, away) == ("A", 1)


def test_ring_of_three_keeps_one_member_resident(driver):
    pol, res, away = driver(list("ABC" * 8))
    assert pol == "111" + "011" * 7
    assert (res, away) == ("A", 2)


def test_fresh_pointers_every_call_always_stream(driver):
    pol, res, _ = driver(["#"] * 40)
    assert pol == "1" * 40
    assert res == "#"


def test_a_replaced_ring_member_hands_residency_over_after_eight_launches(driver):
    # A, B alternate (A resident); then D takes A's place.  After the last launch of A: B D B D B D B D are eight launches
    # that did not write A -- the eighth writes D, which becomes resident; from then on D plain, B streamed.
    seq = list("AB" * 4) + list("DB" * 8)
    pol, res, away = driver(seq)
    assert pol == "11010101" + "11111111" + "01" * 4
    assert (res, away) == ("D", 1)
    # seven such launches are not enough: A, coming back, is still the resident member
    pol, res, away = driver(list("AB" * 4) + list("DBDBDB") + ["A", "B"])
    assert pol == "11010101" + "111111" + "01"
    assert (res, away) == ("A", 1)


def test_a_ring_that_shrinks_to_one_buffer(driver):
    # the streamed member alone: absorbed after the hand-over; the resident member alone: absorbed at once
    pol, res, _ = driver(list("AB" * 3) + list("B" * 12))
    assert pol == "110101" + "1111111" + "00000"
    assert res == "B"
    pol, res, _ = driver(list("AB" * 3) + list("A" * 6))
    assert pol == "110101" + "000000"
    assert res == "A"


def test_size_class_bounds(driver):
    # below 128 MiB: never streams and is never remembered (two such buffers fit the cache together)
    assert driver(list("AAAABABA"), mib=127) == ("0" * 8, "-", 0)
    assert driver(list("AAAABABA"), mib=80) == ("0" * 8, "-", 0)
    # above 256 MiB: always streams, also one buffer rewritten again and again, and is never remembered
    assert driver(list("AAAABABA"), mib=257) == ("1" * 8, "-", 0)
    assert driver(list("AAAA"), mib=20000) == ("1" * 4, "-", 0)
    # both bounds belong to the class
    assert driver(list("AAAA"), mib=128) == ("1000", "A", 0)
    assert driver(list("AAAA"), mib=256) == ("1000", "A", 0)
    # calls outside the class leave what the env remembers alone
    pol, res, away = driver(["A160", "B160", "A160", "C300", "C300", "D64", "A160", "B160"])
    assert pol == "110" + "11" + "0" + "01"
    assert (res, away) == ("A", 1)
