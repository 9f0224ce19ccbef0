"""The decision-complete block corpus: named, seeded cases for the block DSP (oracle/aecm_oracle.c: aecm_oracle_process_block;
webrtc_aecm_amd/csrc/aecm_wave.h: BlockEngine) that between them take every conditional of the block path both ways, except the
ones listed with their reasons in tests/decision_allowlist.json.  tools/decision_coverage.py measures that on the CPU (gcov),
tests/test_decision_coverage.py keeps it true, and tests/test_gpu_block_corpus.py runs every case through every device kernel
family.  Nothing here is recorded audio: every case is generated from its seed.

Four sources: a subset of helpers.adversarial_cases, the bench-shaped pairs of test_lean_block.bench_pair, one stream per
synth profile past both start-up thresholds (512 and 1 024 blocks), and cases written against the coverage report (the second
half of corpus_cases: each says which decision it is there for).  A case is as long as the decision it reaches needs and never
longer than MAX_BLOCKS; most are T_STD = 1 100 blocks."""
from __future__ import annotations

import functools

import numpy as np

from helpers import adversarial_cases, hostile_clean
from webrtc_aecm_amd.synth import EXTRA_PROFILES, PROFILES, synth_pair

T_STD = 1100                    # past CONV_LEN2 = 1 024: all three start-up states
MAX_BLOCKS = 6000
T_NOISE_DEC = 4500              # the comfort-noise estimate needs ~3 300 silent blocks to fall below 2^9 in every bin


def _case(name, far, near, fs, cng, echo_mode, clean=None, path=None, control=None, why=""):
    n = near.size // 64
    assert far.size == near.size == n * 64 and n <= MAX_BLOCKS and (clean is None or clean.size == near.size), name
    return dict(name=name, far=far, near=near, clean=clean, fs=fs, cng=cng, echo_mode=echo_mode, path=path, control=control,
                n_blocks=n, why=why)


def _echo(far, delay, num, den):
    """The far end `delay` samples late, scaled by num / den (integer arithmetic: the same on every machine)."""
    e = np.zeros(far.size, dtype=np.int64)
    e[delay:] = far[:far.size - delay].astype(np.int64) * num // den
    return e


def _i16(x):
    return np.clip(x, -32768, 32767).astype(np.int16)


def _noise(rs, n, amp):
    return rs.randint(-amp, amp + 1, size=n).astype(np.int64)


def _speechlike(rs, n, levels, seg):
    """White noise under a piecewise-constant envelope (levels drawn per `seg` samples), lightly low-passed."""
    env = np.repeat(np.asarray(levels, dtype=np.int64)[rs.randint(0, len(levels), n // seg + 1)], seg)[:n]
    x = rs.randint(-32768, 32768, size=n).astype(np.int64) * env >> 15
    x[1:-1] = (x[:-2] + 2 * x[1:-1] + x[2:]) >> 2
    return x


_SIN_Q15 = np.round(32767 * np.sin(2 * np.pi * np.arange(128) / 128.0)).astype(np.int64)     # exact to the rounding: the same everywhere


def _band_classes(n_blocks, groups1, groups2, change_at, amp=500, seg=4, seed=1):
    """(far, near) of the delay_second_operand case; groups: bands on per class, before / from block change_at."""
    rs = np.random.RandomState(seed)
    ph = rs.randint(0, 128, size=65)
    t = np.arange(n_blocks * 64, dtype=np.int64)
    cls = (t // (64 * seg)) % len(groups1)
    tone = lambda b, shift: (_SIN_Q15[(b * t + ph[b] + shift) % 128] * amp) >> 15
    far = sum(tone(b, 0) for b in range(12, 44)) * (cls == 0)
    near = np.zeros(t.size, dtype=np.int64)
    for groups, when in ((groups1, t < change_at * 64), (groups2, t >= change_at * 64)):
        b = 12
        for c, g in enumerate(groups):
            for k in range(g):
                near += tone(b + k, 20) * ((cls == (c + 1) % len(groups)) & when)
            b += max(g, groups1[c])
    return _i16(far), _i16(near)


def _new_cases():
    """The cases written against the coverage report (profiles/r21_decision_coverage.txt)."""
    # -- the comfort-noise decrement (oracle comfort_noise: noise_est < 2^min_track with the input below the estimate; the
    #    counter behind it is high_ctr, bits 19..21 of the hand-over words): a near end of digital silence / of +-1 dither
    #    under a live far end, cng = 1.  The estimate starts at 2^18 .. 2^20 and falls by 1 / 512 per block.
    rs = np.random.RandomState(2101)
    n = T_NOISE_DEC * 64
    far = _i16(_speechlike(rs, n, [0, 300, 4000, 20000], 3200))
    yield _case("noise_dec_silence", far, np.zeros(n, np.int16), 16000, 1, 3,
                why="comfort-noise decrement: every estimate below 2^9 and above the (zero) input")
    rs = np.random.RandomState(2102)
    far = _i16(_speechlike(rs, n, [0, 300, 4000, 20000], 3200))
    yield _case("noise_dec_dither", far, _i16(_noise(rs, n, 1)), 8000, 1, 1,
                why="comfort-noise decrement next to its increment: +-1 dither keeps some bins above and some below their estimate")
    # the same with a clean input that is silent while the noisy near end is not: the estimator follows the clean spectrum
    rs = np.random.RandomState(2103)
    far = _i16(_speechlike(rs, n, [0, 300, 4000, 20000], 3200))
    near = _i16(_echo(far, 140, 1, 2) + _noise(rs, n, 40))
    yield _case("noise_dec_clean_silence", far, near, 16000, 1, 4, clean=_i16(_noise(rs, n, 1)),
                why="comfort-noise decrement in the clean instantiations")
    # -- the delay estimator's validity test, second operand (best >= minimum_probability, best < last_delay_probability).
    #    Binary spectra by construction: time runs in classes of four blocks, four classes to a period.  The far end has all 32
    #    bands of the estimator (bins 12..43, bin-centred tones) on in class 0, so its binary word is all ones there and 0 (no
    #    update of a mean) elsewhere; the near end has a group of bands on per class, 16 | 6 | 6 | 6: the lags that meet class 0
    #    see 16 differing bits, the others 26 -- a valley of more than PROB_MIN_SPREAD, minimum_probability follows the best mean
    #    down.  From block 800 the first group shrinks to 9 bands: the best mean climbs past minimum_probability while the
    #    valley stays above PROB_OFFSET, and last_delay_probability, one step per block, passes it near block 2 000.
    yield _case("delay_second_operand", *_band_classes(2300, (16, 6, 6, 6), (9, 6, 6, 6), 800), 16000, 1, 3,
                why="validity test of the delay estimator: only its second operand holds")
    # -- start-up state 0 ends while the far end is silent, then a far end at one steady level, later four times louder:
    #    the first far energy above the floor arrives in start-up state 1 (far_energy_min = far_energy_max, the VAD threshold
    #    never set by state 0, the VAD decided by the range test alone)
    rs = np.random.RandomState(2120)
    n = T_STD * 64
    far = np.zeros(n, dtype=np.int64)
    far[530 * 64:] = _noise(rs, n - 530 * 64, 6000)
    far[850 * 64:] = far[850 * 64:] * 4
    near = _echo(far, 200, 1, 3) + _noise(rs, n, 20)
    yield _case("late_far_steady", _i16(far), _i16(near), 16000, 1, 3,
                why="the far-energy trackers are first set after start-up state 0: min = max, VAD from the range test alone")
    yield _case("late_far_steady_clean", _i16(far), _i16(near), 8000, 0, 2, clean=_i16(_echo(far, 200, 1, 5) + _noise(rs, n, 3)),
                why="the same in the clean instantiations")
    # -- no far end at all (suppression gain 0: the pass-through form of the gain) under a clean input whose Q domain steps
    rs = np.random.RandomState(2125)
    n = 300 * 64
    near = _i16(_noise(rs, n, 2000))
    yield _case("far_silent_clean_steps", np.zeros(n, np.int16), near, 16000, 1, 3, clean=hostile_clean(5, near, near, rs),
                why="gain-zero blocks whose clean Q domain moves (q_steady false in the pass-through form)")
    # -- control(): a fixed delay and the NLP switched off, on a converging pair and on a hostile one
    far, near = synth_pair(4201, T_STD, 16000, "mixed")
    yield _case("control_fixed_delay", far, near, 16000, 1, 3, control=(7, 1), why="fixed delay instead of the estimate")
    far, near = synth_pair(4202, T_STD, 8000, "loud")
    yield _case("control_no_nlp", far, near, 8000, 0, 4, control=(-1, 0), why="NLP off")
    # -- level steps of the near end by its whole range from block to block (the Q domain moves up and down), with a clean
    #    input doing the same out of step: near_filt's rescaling and its saturation to 32767
    rs = np.random.RandomState(2130)
    n = T_STD * 64
    far = _i16(_speechlike(rs, n, [0, 40, 3000, 32767], 64))
    near = _i16(_echo(far, 130, 1, 1) + _speechlike(rs, n, [0, 1, 40, 3000, 32767], 64))
    yield _case("level_steps", far, near, 16000, 1, 3, why="Q-domain steps of far and near end from block to block")
    yield _case("level_steps_clean", far, near, 8000, 1, 2, clean=hostile_clean(5, far, near, np.random.RandomState(2131)), control=(-1, 0),
                why="Q-domain steps of the clean input out of step with the noisy one, NLP off")


@functools.lru_cache(maxsize=None)
def _all_cases():
    from test_lean_block import bench_pair
    cases = []
    # 1. hostile inputs: every third adversarial case of the suite's 24 and four more (all six signal kinds, both path kinds, both rates)
    for it, c in enumerate(adversarial_cases(n_cases=24, n_blocks=T_STD)):
        if it % 3 == 1 or it in (0, 5, 6, 15):            # (5 and 15: echo paths with -32768 entries, the negative overflow of ch_adapt32 + step)
            cases.append(_case(f"adversarial{it}", c["far"], c["near"], c["fs"], c["cng"], c["echo_mode"], path=c["path"], why="hostile input"))
    # 2. the bench signal
    for name, seed, prof, fs, cng, em, n in (("bench_recipe", 0, "recipe", 16000, 1, 1, T_STD), ("bench_double_talk", 4, "double_talk", 16000, 1, 1, T_STD),
                                             ("bench_silent", 5, "silent", 16000, 1, 1, 400), ("bench_recipe8k", 6, "recipe", 8000, 0, 3, T_STD)):
        far, near = bench_pair(seed, n, prof)
        cases.append(_case(name, far, near, fs, cng, em, why="bench-shaped signal"))
    # 3. one stream per synth profile, alternating rates, every echo mode, cng 0 among them
    for k, prof in enumerate(PROFILES + EXTRA_PROFILES):
        fs = (16000, 8000)[k % 2]
        far, near = synth_pair(4100 + k, T_STD, fs, prof)
        cases.append(_case(f"synth_{prof}", far, near, fs, 0 if k == 2 else 1, k % 5, why="synth profile past both start-up thresholds"))
    # ... and two with a clean input that is a plain copy / a hostile one
    far, near = synth_pair(4110, T_STD, 16000, "mixed")
    cases.append(_case("synth_clean_copy", far, near, 16000, 1, 3, clean=near.copy(), control=(5, 1), why="clean input = near end, fixed delay"))
    far, near = synth_pair(4111, T_STD, 8000, "sparse")
    cases.append(_case("synth_clean_noise", far, near, 8000, 0, 1, clean=hostile_clean(0, far, near, np.random.RandomState(4111)),
                       why="full-scale noise as the clean input"))
    # 4. written against the coverage report
    cases.extend(_new_cases())
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        for k in ("far", "near", "clean", "path"):
            if c[k] is not None:
                c[k].flags.writeable = False
    return tuple(cases)


def corpus_cases(fs=None, clean=None, without=()):
    """The corpus as a list of dicts: name, far, near, clean (or None), fs, cng, echo_mode, path (int16[65] or None), control
    ((fixed_delay, nlp) or None), n_blocks, why.  fs / clean (True / False) filter; `without`: names left out (the coverage test
    uses it to show that a case is needed).  The arrays are shared and read-only."""
    return [c for c in _all_cases() if (fs is None or c["fs"] == fs) and (clean is None or (c["clean"] is not None) == clean)
            and c["name"] not in without]


def configure(stream, c):
    """Apply a case's echo path and control settings to a block stream (OracleStream, RefCoreStream, SimStream)."""
    if c["path"] is not None:
        stream.init_echo_path(c["path"])
    if c["control"] is not None:
        stream.control(*c["control"])
    return stream
