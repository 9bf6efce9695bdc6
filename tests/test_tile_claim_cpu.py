"""The fast kernels' tile hand-out (fqtool_amd/csrc/tile_claim.h: a strided body, a claimed tail),
without a GPU: tools/micro/tile_claim_sim.cpp runs the kernel's loop for W simulated waves under
AddressSanitizer / UBSan and fails unless every tile of [0, ntiles) is run exactly once and none
beyond.  The header's kClaimTiles is the one kept claim step."""
import os
import re
import subprocess

import pytest

from fqtool_amd import abi

SIM_SRC = os.path.join(abi.REPO_DIR, "tools", "micro", "tile_claim_sim.cpp")


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """The program built by the compile line in its own header."""
    head = open(SIM_SRC).read().split("#include")[0]
    line = next(l for l in head.splitlines() if "g++ " in l)
    argv = line[line.index("g++"):].split()
    assert argv[:5] == ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined"]
    binary = str(tmp_path_factory.mktemp("claim") / "tile_claim_sim")
    argv[argv.index("-o") + 1] = binary
    subprocess.run(argv, check=True, cwd=abi.REPO_DIR)
    return binary


def sizes(W):
    return [0, 1, W - 1, W, W + 1, 10 * W + 17, 763 * W + 5]


@pytest.mark.parametrize("W", [16, 4096])
def test_every_tile_once(sim, W):
    for ntiles in sizes(W):
        for seed in (1, 2):
            r = subprocess.run([sim, str(W), str(ntiles), str(seed)], capture_output=True, text=True)
            assert r.returncode == 0, (W, ntiles, seed, r.stdout, r.stderr)
            assert r.stderr == "", r.stderr  # (no sanitizer report)
            m = re.match(r"W (\d+) ntiles (\d+) T0 (\d+) claims (\d+) makespan (\d+) fixed (\d+) bad 0\n$", r.stdout)
            assert m, r.stdout
            t0, claims = int(m.group(3)), int(m.group(4))
            # the split the kernels' host side computes: whole rounds below T0, a tail of at least
            # one round (the whole batch when it is smaller), at most an eighth of the tiles + a round
            assert t0 % W == 0 and 0 <= t0 <= ntiles
            assert ntiles - t0 >= min(ntiles, W)
            assert ntiles - t0 < max(W, ntiles // 8) + W
            # every wave's last claim fails, the others each hand out a run of tiles
            assert claims >= W and claims <= (ntiles - t0) + W


def test_small_batch_is_all_claimed_and_ten_rounds_use_both(sim):
    out = subprocess.run([sim, "4096", "4097", "3"], capture_output=True, text=True, check=True).stdout
    assert " T0 0 " in out
    out = subprocess.run([sim, "4096", str(10 * 4096 + 17), "3"], capture_output=True, text=True, check=True).stdout
    assert " T0 %d " % (8 * 4096) in out


def test_claimed_tail_shortens_the_makespan(sim):
    """With uneven tiles and waves the claimed tail ends no later than the fixed stride."""
    out = subprocess.run([sim, "4096", str(763 * 4096 + 5), "7"], capture_output=True, text=True, check=True).stdout
    m = re.search(r"makespan (\d+) fixed (\d+)", out)
    assert int(m.group(1)) <= int(m.group(2))
