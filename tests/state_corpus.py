"""The seeded state corpus: state images (webrtc_aecm_amd/csrc/aecm_state.h) to START a block stream from -- states the algorithm
reached, and mutations of them the algorithm can never reach but the import gate (webrtc_aecm_amd/csrc/aecm_state_check.h) admits.
tests/test_state_injection.py runs every admitted one on the lane simulator with the claims of aecm_ops.h checked and against the
oracle (oracle/aecm_oracle.c: aecm_oracle_import_image); tests/test_gpu_state_injection.py imports them into the device.

STATE_RULES restates the gate by hand, from the reference's member types (aecm/aecm_core.h:41-141, aecm/delay_estimator.h:22-63)
and from what its own code can leave in a member.  It is NOT parsed from the header: the tests hold restatement = product on every
blob generated here, so a rule dropped or loosened on either side shows.

An image is (vec uint32[12 * 64], scal int32[64], hist uint16[100 * 64]); a State adds the rate, a name and whether its
continuation audio comes with a clean near-end input.  Nothing here is recorded: everything is generated from seeds."""
from __future__ import annotations

import functools
import struct
from dataclasses import dataclass

import numpy as np

LANES, N_VEC, N_SCAL, HISTORY = 64, 12, 64, 100
VEC_WORDS, HIST_WORDS = N_VEC * LANES, HISTORY * LANES
SECOND, LOGS = 36, 20                         # MAX_DELAY - 64; MIN_MSE_COUNT (aecm_core.cc:943-952)
I16 = (-32768, 32767)
I32_MAX = 2 ** 31 - 1

VEC_NAMES = ("V_XD_OLD", "V_OUTBUF", "V_CH16", "V_CH32", "V_ECHOFILT", "V_NEARFILT", "V_NOISE", "V_MEAN", "V_BH0", "V_BH1", "V_M01", "V_HQ")
V = {n: i for i, n in enumerate(VEC_NAMES)}
SCAL_NAMES = ("S_TOTCOUNT", "S_SEED", "S_STARTUP", "S_HISTPOS", "S_DFANOISYQ", "S_DFANOISYQ_OLD", "S_DFACLEANQ", "S_DFACLEANQ_OLD",
              "S_FARLOG", "S_FE_MIN", "S_FE_MAX", "S_FE_MAXMIN", "S_FE_VAD", "S_FE_MSE", "S_CURVAD", "S_VADCNT", "S_FIRSTVAD", "S_MSECNT",
              "S_MSE_ADAPT_OLD", "S_MSE_STORED_OLD", "S_MSE_THRESH", "S_SUPGAIN", "S_SUPGAIN_OLD", "S_NOISECTR",
              "S_FAR_INIT", "S_NEAR_INIT", "S_MIN_PROB", "S_LAST_PROB", "S_LAST_DELAY",
              "S_MULT", "S_CNG", "S_NLP", "S_FIXED_DELAY", "S_SG_A", "S_SG_D", "S_SG_DAB", "S_SG_DBD",
              "S_B64_CHSTORED", "S_B64_CHADAPT16", "S_B64_CHADAPT32", "S_B64_ECHOFILT", "S_B64_NEARFILT", "S_B64_NOISE", "S_B64_LOWCTR",
              "S_B64_HIGHCTR")
S = {n: i for i, n in enumerate(SCAL_NAMES)}
N_SCAL_USED = len(SCAL_NAMES)

# snapshot blob (include/aecm_batch.h: WebRtcAecmBatch_ExportState): 8 header words, then vec, scal, hist as they lie in memory
HEADER_BYTES = 32
BLOB_BYTES = HEADER_BYTES + VEC_WORDS * 4 + N_SCAL * 4 + HIST_WORDS * 2
MAGIC, LAYOUT_VERSION = 0x53434541, 3


@dataclass(frozen=True)
class Rule:
    """field holds a value in [lo, hi] (lo / hi: numbers or functions of the rate).  Scalar rule: `field` is a SCAL_NAMES entry.
    Lane rule: `field` is a VEC_NAMES entry, the value is the `width` bits from bit `shift` of the word (signed when the whole
    word), and the rule holds in the lanes where lanes(t)."""
    name: str
    field: str
    lo: object
    hi: object
    defect: str
    shift: int = 0
    width: int = 32
    lanes: object = None

    @property
    def is_lane(self):
        return self.field in V

    def bounds(self, fs):
        return tuple(b(fs) if callable(b) else b for b in (self.lo, self.hi))

    def applies(self, t):
        return self.lanes is None or self.lanes(t)

    def representable(self):
        """(min, max) the storage can hold."""
        if self.width == 32:
            return -2 ** 31, I32_MAX
        return 0, (1 << self.width) - 1


def _i16_rule(field):
    return Rule(field, field, *I16, "int16 member")


STATE_RULES = (
    # ---- scalars, in the order of the scalar block ----
    Rule("S_SEED", "S_SEED", 0, I32_MAX, "seed"),                                # WebRtcSpl_RandUN masks the LCG to 31 bits (spl.cc:129-147)
    Rule("S_STARTUP", "S_STARTUP", 0, 2, "startupState"),                          # (totCount >= 512) + (totCount >= 1024), aecm_core_c.cc:420-424
    Rule("S_HISTPOS", "S_HISTPOS", 0, HISTORY, "far_history_pos"),                 # MAX_DELAY after init (aecm_core.cc:397), then 0..99 (:125-138)
    Rule("S_DFANOISYQ", "S_DFANOISYQ", 0, 14, "dfaQDomain"),                       # WebRtcSpl_NormW16 of a non-negative int16 (spl_inl.h:108)
    Rule("S_DFANOISYQ_OLD", "S_DFANOISYQ_OLD", 0, 14, "dfaQDomain"),
    Rule("S_DFACLEANQ", "S_DFACLEANQ", 0, 14, "dfaQDomain"),
    Rule("S_DFACLEANQ_OLD", "S_DFACLEANQ_OLD", 0, 14, "dfaQDomain"),
    _i16_rule("S_FARLOG"), _i16_rule("S_FE_MIN"), _i16_rule("S_FE_MAX"), _i16_rule("S_FE_MAXMIN"), _i16_rule("S_FE_VAD"), _i16_rule("S_FE_MSE"),
    Rule("S_CURVAD", "S_CURVAD", 0, 1, "flag"),                                    # aecm_core.cc:733-740
    _i16_rule("S_VADCNT"),
    Rule("S_FIRSTVAD", "S_FIRSTVAD", 0, 1, "flag"),                                # aecm_core.cc:741-754
    _i16_rule("S_MSECNT"),
    Rule("S_SUPGAIN", "S_SUPGAIN", 0, 32767, "supGain"),                           # int16, smoothed maximum of non-negative targets (aecm_core.cc:1000-1052)
    _i16_rule("S_SUPGAIN_OLD"), _i16_rule("S_NOISECTR"),
    Rule("S_FAR_INIT", "S_FAR_INIT", 0, 1, "flag"),                                # delay_estimator_wrapper.cc:92-125
    Rule("S_NEAR_INIT", "S_NEAR_INIT", 0, 1, "flag"),
    Rule("S_MIN_PROB", "S_MIN_PROB", 0, I32_MAX, "delay probability"),             # Q9 bit counts and thresholds of them (delay_estimator.cc:593-609)
    Rule("S_LAST_PROB", "S_LAST_PROB", 0, I32_MAX, "delay probability"),
    Rule("S_LAST_DELAY", "S_LAST_DELAY", -2, HISTORY - 1, "last_delay"),           # -2 after init, then a history slot (delay_estimator.cc:643-661)
    Rule("S_MULT", "S_MULT", lambda fs: fs // 8000, lambda fs: fs // 8000, "mult"),   # aecm_core.cc:368
    Rule("S_CNG", "S_CNG", 0, 1, "cngMode"),                                       # echo_control_mobile.cc:416-418
    _i16_rule("S_NLP"),                                                            # aecm_core.cc:477-482: Control stores int16
    Rule("S_FIXED_DELAY", "S_FIXED_DELAY", -32768, HISTORY - 1, "fixedDelay"),     # an index into the far history when >= 0 (aecm_core_c.cc:485-488)
    _i16_rule("S_SG_A"), _i16_rule("S_SG_D"), _i16_rule("S_SG_DAB"), _i16_rule("S_SG_DBD"),
    _i16_rule("S_B64_CHSTORED"), _i16_rule("S_B64_CHADAPT16"), _i16_rule("S_B64_NEARFILT"),
    Rule("S_B64_NOISE", "S_B64_NOISE", 0, I32_MAX, "noiseEst[64]"),                # starts positive, never updated below 0 (aecm_core_c.cc:81-127)
    Rule("S_B64_LOWCTR", "S_B64_LOWCTR", 0, 7, "noiseEstCtr[64]"),                 # three bits in the lane words; the algorithm keeps it < 5
    Rule("S_B64_HIGHCTR", "S_B64_HIGHCTR", 0, 7, "noiseEstCtr[64]"),
    # ---- lane words ----
    Rule("far_q_domains[t]", "V_NEARFILT", 0, 14, "far_q_domains", shift=22, width=5),
    Rule("far_q_domains[t+64]", "V_NEARFILT", 0, 14, "far_q_domains", shift=27, width=5, lanes=lambda t: t < SECOND),
    Rule("noiseEst[t]", "V_NOISE", 0, I32_MAX, "noiseEst"),
    # thresholds of the binary spectra: 0 at init (delay_estimator_wrapper.cc:208-225, 338-355), then moved part of the way towards
    # spectrum << (15 - q) in [0, 2^31) (:92-125, delay_estimator.cc:690) -- found by tests/test_state_injection.py: with a negative
    # threshold new_value - mean overflows, which the reference leaves undefined
    Rule("mean_spectrum[t]", "V_MEAN", 0, I32_MAX, "mean_spectrum"),
    Rule("mean_bit_counts[t]", "V_M01", 0, 32 << 9, "mean_bit_counts", shift=0, width=16),     # Q9 means of counts of 32 bits (delay_estimator.h)
    Rule("mean_bit_counts[t+64]", "V_M01", 0, 32 << 9, "mean_bit_counts", shift=16, width=16, lanes=lambda t: t < SECOND),
    Rule("no slot t+64", "V_M01", 0, 0, "mean_bit_counts", shift=16, width=16, lanes=lambda t: t >= SECOND),
)
# The rule over several fields: supGainErrParamA, D, DiffAB, DiffBD are written by WebRtcAecm_set_config alone, as one of five tuples
# (echo_control_mobile.cc:424-476 from aecm_defines.h:62-68: A 3072, B 1536, D 256, shifted right by 3 - echoMode or left by 1)
SG_FIELDS = ("S_SG_A", "S_SG_D", "S_SG_DAB", "S_SG_DBD")
SG_TUPLES = tuple((a, d, a - b, b - d) for a, b, d in ((3072 >> 3, 1536 >> 3, 256 >> 3), (3072 >> 2, 1536 >> 2, 256 >> 2), (3072 >> 1, 1536 >> 1, 256 >> 1),
                                                        (3072, 1536, 256), (3072 << 1, 1536 << 1, 256 << 1)))
SG_DEFECT = "supGainErrParam"

SCALAR_RULES = {r.field: r for r in STATE_RULES if not r.is_lane}
LANE_RULES = tuple(r for r in STATE_RULES if r.is_lane)
assert len(SCALAR_RULES) + len(LANE_RULES) == len(STATE_RULES)
# what no rule covers (mutation class b): the int32 members among the scalars, and the lane words that are plain data
UNCHECKED_SCALARS = tuple(n for n in SCAL_NAMES if n not in SCALAR_RULES)
UNCHECKED_VEC = ("V_CH16", "V_CH32", "V_ECHOFILT", "V_BH0", "V_BH1", "V_HQ", "V_XD_OLD", "V_OUTBUF")
assert UNCHECKED_SCALARS == ("S_TOTCOUNT", "S_MSE_ADAPT_OLD", "S_MSE_STORED_OLD", "S_MSE_THRESH", "S_B64_CHADAPT32", "S_B64_ECHOFILT")


def lane_value(rule, word):
    word = int(word)
    if rule.width == 32:
        return word - (1 << 32) if word & 0x80000000 else word
    return (word >> rule.shift) & ((1 << rule.width) - 1)


def with_lane_value(rule, word, value):
    if rule.width == 32:
        return value & 0xffffffff
    mask = ((1 << rule.width) - 1) << rule.shift
    return (int(word) & ~mask & 0xffffffff) | ((value << rule.shift) & mask)


def restated_defect(vec, scal, fs):
    """The verdict STATE_RULES gives, in the order the product reports defects: scalar fields by index, the rule over the four
    supGainErrParam words, then lane by lane (the nearFilt word, the noise word, the threshold word, the bit-count word).  None = admitted."""
    for name in SCAL_NAMES:
        r = SCALAR_RULES.get(name)
        if r is not None:
            lo, hi = r.bounds(fs)
            if not lo <= int(scal[S[name]]) <= hi:
                return r.defect
    if tuple(int(scal[S[n]]) for n in SG_FIELDS) not in SG_TUPLES:
        return SG_DEFECT
    for t in range(LANES):
        for r in LANE_RULES:
            if r.applies(t):
                lo, hi = r.bounds(fs)
                if not lo <= lane_value(r, vec[V[r.field] * LANES + t]) <= hi:
                    return r.defect
    return None


# ---- the words no member owns --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def live_masks():
    """(vec uint32[12 * 64], scal int32[64] as uint32): the bits of an image some member owns.  The rest -- lanes 56..63 of V_BH1 and
    of the upper half of V_HQ, bits 27..31 of V_NEARFILT in lanes 36..63, scal[45..63] -- are dead: a launch may leave anything
    there (the kernels write 0), the oracle exports 0.  The upper half of V_M01 in lanes 36..63 is no member's either, but the gate
    holds it to 0 (the kernels add it up with the rest), so it counts as live.  Every history word is live."""
    vec = np.full((N_VEC, LANES), 0xffffffff, dtype=np.uint32)
    vec[V["V_BH1"], SECOND + LOGS:] = 0
    vec[V["V_HQ"], SECOND + LOGS:] = 0x0000ffff
    vec[V["V_NEARFILT"], SECOND:] = 0x07ffffff
    scal = np.zeros(N_SCAL, dtype=np.uint32)
    scal[:N_SCAL_USED] = 0xffffffff
    for a in (vec, scal):
        a.flags.writeable = False
    return vec.reshape(-1), scal


def _vec_word_name(i):
    f, t = divmod(int(i), LANES)
    return f"{VEC_NAMES[f]}[lane {t}]"


def describe_image_diff(a, b, live_only=True, limit=8):
    """'' when the images a and b ((vec, scal, hist) each) are equal -- on the live words with live_only --, else the first
    `limit` differing words by field and lane."""
    vm, sm = live_masks() if live_only else (np.uint32(0xffffffff), np.uint32(0xffffffff))
    av, bv = (np.asarray(x[0], dtype=np.uint32).reshape(-1) & vm for x in (a, b))
    as_, bs = (np.asarray(x[1], dtype=np.int32).reshape(-1).view(np.uint32) & sm for x in (a, b))
    ah, bh = (np.asarray(x[2], dtype=np.uint16).reshape(-1) for x in (a, b))
    lines = []
    for i in np.flatnonzero(av != bv):
        lines.append(f"{_vec_word_name(i)}: {int(av[i]):#010x} != {int(bv[i]):#010x}")
    for i in np.flatnonzero(as_ != bs):
        name = SCAL_NAMES[i] if i < N_SCAL_USED else f"scal[{i}] (dead)"
        lines.append(f"{name}: {int(as_[i].astype(np.int32))} != {int(bs[i].astype(np.int32))}")
    for i in np.flatnonzero(ah != bh):
        lines.append(f"far_history[slot {i // LANES}][bin {i % LANES}]: {int(ah[i])} != {int(bh[i])}")
    more = len(lines) - limit
    return "; ".join(lines[:limit]) + (f"; ... {more} more" if more > 0 else "")


# ---- states --------------------------------------------------------------------------------------------------------------------
@dataclass
class State:
    name: str
    fs: int
    vec: np.ndarray
    scal: np.ndarray
    hist: np.ndarray
    clean: bool = False            # run the continuation with the clean near-end input

    def copy(self, name=None):
        return State(name or self.name, self.fs, self.vec.copy(), self.scal.copy(), self.hist.copy(), self.clean)

    @property
    def image(self):
        return self.vec, self.scal, self.hist

    def expected_defect(self):
        return restated_defect(self.vec, self.scal, self.fs)

    def blob(self):
        """The snapshot blob of this image (what WebRtcAecmBatch_ExportState writes)."""
        return (struct.pack("<8I", MAGIC, LAYOUT_VERSION, self.fs, N_VEC, N_SCAL, HISTORY, LANES, 0) + self.vec.astype("<u4").tobytes() +
                self.scal.astype("<i4").tobytes() + self.hist.astype("<u2").tobytes())


def image_of_blob(blob):
    b = bytes(blob)
    assert len(b) == BLOB_BYTES
    at = HEADER_BYTES
    vec = np.frombuffer(b, "<u4", VEC_WORDS, at).astype(np.uint32)
    scal = np.frombuffer(b, "<i4", N_SCAL, at + VEC_WORDS * 4).astype(np.int32)
    hist = np.frombuffer(b, "<u2", HIST_WORDS, at + VEC_WORDS * 4 + N_SCAL * 4).astype(np.uint16)
    return vec, scal, hist


AGES = (0, 40, 700, 1300)          # blocks: fresh, start-up state 0, state 1 (>= 512), state 2 (>= 1024) with everything converged
# (rate, cng, echo mode, audio, fixed delay or None, clean input): both rates, every echo mode, comfort noise on and off, quiet and
# full-scale audio, a fixed delay, with and without a clean near-end input
BASE_CONFIGS = (
    (16000, 1, 3, "mixed", None, False), (8000, 1, 0, "steady", None, False), (16000, 0, 1, "loud", None, True), (8000, 1, 2, "quiet", None, True),
    (16000, 1, 4, "fullscale", None, False), (8000, 0, 4, "fullscale", None, True), (16000, 1, 3, "mixed", 7, True), (8000, 0, 3, "quiet", 42, False),
    (16000, 1, 2, "sparse", None, False), (8000, 1, 1, "silent", None, False),
)


def _base_audio(kind, seed, n_blocks, fs):
    from webrtc_aecm_amd.synth import synth_clean, synth_pair
    rs = np.random.RandomState(seed)
    n = n_blocks * 64
    if kind == "quiet":
        far = rs.randint(-40, 41, size=n).astype(np.int16)
        near = (np.roll(far, 90) // 2 + rs.randint(-3, 4, size=n)).astype(np.int16)
    elif kind == "fullscale":
        far = rs.randint(-32768, 32768, size=n).astype(np.int16)
        near = np.clip(np.roll(far, 120).astype(np.int64) + rs.randint(-32768, 32768, size=n), -32768, 32767).astype(np.int16)
    else:
        far, near = synth_pair(seed, n_blocks, fs, kind)
    return far, near, synth_clean(near) if kind != "fullscale" else rs.randint(-32768, 32768, size=n).astype(np.int16)


@functools.lru_cache(maxsize=None)
def base_states():
    """Reachable states: every BASE_CONFIGS entry on the lane simulator at the AGES.  All of them are admitted by construction
    (tests/test_state_injection.py checks it)."""
    import simlib
    out = []
    for k, (fs, cng, em, kind, fixed, clean) in enumerate(BASE_CONFIGS):
        s = simlib.SimStream(fs, cng, em)
        if fixed is not None:
            s.control(fixed, 1)
        far, near, cl = _base_audio(kind, 7300 + k, AGES[-1], fs)
        done = 0
        for age in AGES:
            if age > done:
                sl = slice(done * 64, age * 64)
                s.process(far[sl], near[sl], cl[sl] if clean else None)
                done = age
            vec, scal, hist = s.image()
            out.append(State(f"base{k}_{kind}_fs{fs}_cng{cng}_em{em}{'_fixed' if fixed is not None else ''}{'_clean' if clean else ''}_age{age}",
                             fs, vec, scal, hist, clean))
    return tuple(out)


N_BLOCKS = 6
LAUNCHES = (1, 2, 3)               # the six continuation blocks as three launches


def continuation_audio(index, n_blocks=N_BLOCKS):
    """(far, near, clean) int16[n_blocks * 64] for the state at `index` of a list: levels drawn per block among silence, a few
    units, speech level and full scale, the near end an echo of the far end plus talk of its own level, the clean input on its own."""
    rs = np.random.RandomState(0x5eed0000 + index)
    n = n_blocks * 64
    levels = np.array([0, 3, 300, 8000, 32768], dtype=np.int64)

    def sig():
        env = np.repeat(levels[rs.randint(0, len(levels), size=n_blocks)], 64)
        return rs.randint(-32768, 32768, size=n).astype(np.int64) * env >> 15
    far = sig()
    near = np.roll(far, 17) * int(rs.randint(0, 3)) // 2 + sig()
    clean = sig()
    return tuple(np.clip(x, -32768, 32767).astype(np.int16) for x in (far, near, clean))


# ---- mutations -----------------------------------------------------------------------------------------------------------------
RULE_LANES = (0, 35, 36, 63)       # the lanes a lane rule is probed at: both ends, and both sides of the second-pass boundary


def set_rule_value(state, rule, value, lane=0):
    if rule.is_lane:
        i = V[rule.field] * LANES + lane
        state.vec[i] = with_lane_value(rule, state.vec[i], value)
    else:
        state.scal[S[rule.field]] = value


def rule_probes(fs):
    """Every rule x {lo - 1, lo, hi, hi + 1} (lane rules: at each of RULE_LANES where the rule holds) as (rule, lane, value,
    admitted); a value the storage cannot hold (below 0 in a bit field, beyond int32) is left out."""
    for r in STATE_RULES:
        lo, hi = r.bounds(fs)
        rmin, rmax = r.representable()
        for lane in (RULE_LANES if r.is_lane else (0,)):
            if not r.applies(lane):
                continue
            for value, ok in ((lo - 1, False), (lo, True)) + (((hi, True),) if hi != lo else ()) + ((hi + 1, False),):
                if rmin <= value <= rmax:
                    yield r, lane, value, ok


def sg_probes():
    """The rule over the four supGainErrParam words as (tuple, admitted): the five tuples, each word of each one off by one, and
    words of different tuples mixed."""
    for k, tup in enumerate(SG_TUPLES):
        yield tup, True
        for i in range(4):
            for d in (-1, 1):
                yield tuple(v + d if j == i else v for j, v in enumerate(tup)), False
        other = SG_TUPLES[(k + 1) % len(SG_TUPLES)]
        for i in range(4):
            yield tuple(other[j] if j == i else v for j, v in enumerate(tup)), False


def _pick_base(k, fs=None):
    bases = [b for b in base_states() if fs is None or b.fs == fs]
    return bases[k % len(bases)]


@functools.lru_cache(maxsize=None)
def rule_mutations():
    """Class (a): one State per probe of rule_probes / sg_probes, on base states of both rates in turn.  A lane-rule probe that
    is admitted keeps the base state's other fields, so the state as a whole is admitted exactly when the probe is -- except the
    four supGainErrParam words, whose int16 bounds are no tuple (sg_probes covers what is admitted there)."""
    out = []
    k = 0
    for fs in (16000, 8000):
        for r, lane, value, ok in rule_probes(fs):
            base = _pick_base(k, fs)
            k += 1
            st = base.copy(f"{r.name}{f'@lane{lane}' if r.is_lane else ''}={value}|{base.name}")
            set_rule_value(st, r, value, lane)
            out.append(st)
    for tup, ok in sg_probes():
        base = _pick_base(k)
        k += 1
        st = base.copy(f"supGainErrParam={tup}|{base.name}")
        for n, v in zip(SG_FIELDS, tup):
            st.scal[S[n]] = v
        out.append(st)
    return tuple(out)


INDEX_PROBES = (("S_HISTPOS", 0), ("S_HISTPOS", 100), ("S_LAST_DELAY", -2), ("S_LAST_DELAY", 99), ("S_FIXED_DELAY", -32768), ("S_FIXED_DELAY", 99))
_WORD_EXTREMES = (0x00000000, 0xffffffff, 0x7fffffff, 0x80000000, 0x7fff8000, 0x80007fff)


@functools.lru_cache(maxsize=None)
def extreme_mutations():
    """Class (b): every word no rule covers at its type's extremes -- the int32 members among the scalars, the plain-data lane
    words (all lanes at once, and lane 0 / 63 alone), history rows of 0xffff (all rows, the row at the write position, the row
    the delay points at) -- and the index-like fields at both ends of their ranges on states old enough to have a full history."""
    out = []
    k = 0
    old = [b for b in base_states() if b.name.endswith(("age700", "age1300"))]

    def nxt():
        nonlocal k
        k += 1
        return old[k % len(old)]
    for name in UNCHECKED_SCALARS:
        for value in (-2 ** 31, -1, 0, 1, I32_MAX):
            base = nxt()
            st = base.copy(f"{name}={value}|{base.name}")
            st.scal[S[name]] = value
            out.append(st)
    for name in UNCHECKED_VEC:
        for value in _WORD_EXTREMES:
            for lanes in (slice(0, LANES), slice(0, 1), slice(63, 64)):
                base = nxt()
                st = base.copy(f"{name}[{lanes.start}:{lanes.stop}]={value:#x}|{base.name}")
                st.vec[V[name] * LANES + lanes.start:V[name] * LANES + lanes.stop] = value
                out.append(st)
    for which in ("all", "write", "aligned"):
        for value in (0xffff, 0x8000):
            base = nxt()
            st = base.copy(f"far_history[{which}]={value:#x}|{base.name}")
            pos = int(st.scal[S["S_HISTPOS"]]) % HISTORY
            rows = {"all": range(HISTORY), "write": [(pos + 1) % HISTORY], "aligned": [(pos + 1 - max(int(st.scal[S["S_LAST_DELAY"]]), 0)) % HISTORY]}[which]
            for p in rows:
                st.hist[p * LANES:(p + 1) * LANES] = value
            out.append(st)
    for name, value in INDEX_PROBES:
        for _ in range(2):
            base = nxt()
            st = base.copy(f"{name}={value}|{base.name}")
            st.scal[S[name]] = value
            out.append(st)
    return tuple(out)


def _interesting(rs, lo, hi, rmin, rmax):
    """A value for a field with the admitted range [lo, hi] in storage [rmin, rmax]: mostly inside (the ends and near them more
    often than the middle), sometimes just outside or anywhere."""
    c = rs.randint(0, 20)
    if c < 4:
        return lo if c < 2 else hi
    if c < 8:
        return int(np.clip((lo, hi)[c & 1] + (1, -1)[c & 1] * int(rs.randint(0, 4)), lo, hi))
    if c < 16:
        return int(rs.randint(lo, hi + 1, dtype=np.int64))
    if c < 18:
        return int(np.clip((lo - 1, hi + 1)[c & 1], rmin, rmax))
    return int(rs.randint(rmin, rmax + 1, dtype=np.int64))


def single_field_mutations(seed, count):
    """`count` seeded mutations of ONE field each of a base state (a scalar member, one lane's part of a lane word, one history
    word): States, admitted or not -- ask expected_defect()."""
    rs = np.random.RandomState(seed)
    bases = base_states()
    out = []
    for n in range(count):
        base = bases[rs.randint(0, len(bases))]
        st = base.copy()
        c = rs.randint(0, 10)
        if c < 4:                                                          # a scalar member
            name = SCAL_NAMES[rs.randint(0, N_SCAL_USED)]
            if name in SG_FIELDS:                                          # a word of the tuple alone is never admitted: move the tuple
                tup = SG_TUPLES[rs.randint(0, len(SG_TUPLES))] if rs.randint(0, 8) else tuple(int(v) for v in rs.randint(-32768, 32768, size=4))
                for f, v in zip(SG_FIELDS, tup):
                    st.scal[S[f]] = v
                what = f"supGainErrParam={tup}"
            else:
                r = SCALAR_RULES.get(name)
                lo, hi = r.bounds(st.fs) if r else (-2 ** 31, I32_MAX)
                value = _interesting(rs, lo, hi, -2 ** 31, I32_MAX)
                st.scal[S[name]] = value
                what = f"{name}={value}"
        elif c < 9:                                                        # one lane of a lane word
            f, t = int(rs.randint(0, N_VEC)), int(rs.randint(0, LANES))
            i = f * LANES + t
            rules = [r for r in LANE_RULES if r.field == VEC_NAMES[f] and r.applies(t)]
            if rules and rs.randint(0, 4):
                r = rules[rs.randint(0, len(rules))]
                value = _interesting(rs, *r.bounds(st.fs), *r.representable())
                st.vec[i] = with_lane_value(r, st.vec[i], value)
                what = f"{r.name}@lane{t}={value}"
            else:
                word = _WORD_EXTREMES[rs.randint(0, len(_WORD_EXTREMES))] if rs.randint(0, 2) else int(rs.randint(0, 2 ** 32, dtype=np.int64))
                if rules:                                                  # keep the ruled parts of the word: this mutation is about the rest
                    for r in rules:
                        word = with_lane_value(r, word, lane_value(r, st.vec[i])) if r.width < 32 else int(st.vec[i])
                st.vec[i] = word
                what = f"{VEC_NAMES[f]}@lane{t}={word:#x}"
        else:                                                              # one history word
            i = int(rs.randint(0, HIST_WORDS))
            value = (0xffff, 0x8000, 0, int(rs.randint(0, 65536)))[rs.randint(0, 4)]
            st.hist[i] = value
            what = f"far_history[{i // LANES}][{i % LANES}]={value}"
        st.name = f"m{seed}.{n}:{what}|{base.name}"
        if rs.randint(0, 3) == 0:
            st.clean = True
        out.append(st)
    return out


def combination_mutations(seed, count):
    """Class (c): 2..6 single-field mutations on top of each other."""
    rs = np.random.RandomState(seed)
    out = []
    for n in range(count):
        k = int(rs.randint(2, 7))
        parts = single_field_mutations(int(rs.randint(0, 2 ** 31 - 1)), k)
        st = parts[0]
        base = next(b for b in base_states() if st.name.endswith("|" + b.name))
        for p in parts[1:]:                                                # the words p changed against ITS base, applied to st
            pb = next(b for b in base_states() if p.name.endswith("|" + b.name))
            for mine, theirs, orig in ((st.vec, p.vec, pb.vec), (st.scal, p.scal, pb.scal), (st.hist, p.hist, pb.hist)):
                changed = theirs != orig
                mine[changed] = theirs[changed]
        st.name = f"c{seed}.{n}:" + "+".join(p.name.split(":", 1)[1].split("|")[0] for p in parts) + "|" + base.name
        out.append(st)
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    """Base states, class (a), class (b) and 600 of class (c): the fixed part of the corpus, admitted and refused ones alike."""
    return tuple(base_states()) + rule_mutations() + extreme_mutations() + tuple(combination_mutations(20260, 600))


def stack(states):
    """(vec [n, 768], scal [n, 64], hist [n, 6400]) copies of the states' images."""
    return (np.stack([s.vec for s in states]).astype(np.uint32), np.stack([s.scal for s in states]).astype(np.int32),
            np.stack([s.hist for s in states]).astype(np.uint16))
