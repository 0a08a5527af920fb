"""Schedules for the multirate history tests and a model of the history INDICES (no arithmetic).

The model restates, in plain Python, which entry a correcting filter restarts its chain from (k_step_mr, ekf_multirate.hpp: anchor,
grid checkpoint or the extra checkpoint), how the host places the extra checkpoint (mr_schedule_extra, mr_ck_for_predict and the reset
in mr_prepare, ekf_host.hpp / ekf_capi.hip), and the tick-origin shift (advance_tick).  It is driven by which filters performed a
correction on which tick -- the oracle's Filter.filter_update decides that -- and gives every correcting lane-tick a class, so that a
test can COUNT what a schedule reached instead of trusting a random generator to reach it:

  A   anchor start, clamped: the history is no longer than the step delay (mt == first)
  B   anchor start with a pre-replay
  C0  grid-checkpoint start, no pre-replay (mt % k == 0)
  C+  grid-checkpoint start with a pre-replay
  D   extra-slot start at mt, in a wave where every valid lane corrects and starts at its entry (the fp32 `early` path)
  E   extra-slot start with a pre-replay of 1-2 ticks
  F   extra slot filled for this frame but e_tick > mt: fallback to the grid or the anchor
  G   extra slot filled for this frame but not newer than the lane's anchor or grid start
  H   extra-slot start at mt in a wave where `early` does not hold
  Jg / Je  the start slot (grid / extra) was last written by a correction's replay, not by a predict launch
  K   the chain reads IMU ring slots on both sides of slot 0;  Kg: the grid start slot's index has been reused since seeding
  La / Lu  a tick-origin shift between arming and filling the extra slot / between filling and using it
"""
import numpy as np

WAVE = 64
B_SCHED = 64 + 64 + 37         # two full waves and a ragged one
DT = 0.01                      # update_freq = 100 Hz
OFFSET = 0.001                 # dyn_measurement_delay_offset of the dynamic modes
CLASSES = ("A", "B", "C0", "C+", "D", "E", "F", "G", "H", "Jg", "Je", "K", "Kg", "La", "Lu")
NEVER = -(1 << 30)


def floor_div(a, b):
    return a // b              # Python's // floors, like floor_div of ekf_multirate.hpp


def history_sizes(step_max, k):
    """Nc grid checkpoint slots and Cu = k Nc IMU ring slots (qle_set_params)."""
    Nc = (step_max + k + 1 + k - 1) // k + 1
    return Nc, Nc * k


def choose_start(first, tick, step, k, e_tick):
    """(mt, start, kind) of a correcting lane, kind in 'anchor' / 'grid' / 'extra' (ekf_multirate.hpp, `if (corr)` block)."""
    ind = max(tick - first - step, 0)
    mt = first + ind
    c0 = floor_div(mt, k) * k
    start, kind = (c0, "grid") if c0 > first else (first, "anchor")
    if e_tick > start and e_tick <= mt:
        start, kind = e_tick, "extra"
    return mt, start, kind


def choose_start_bruteforce(first, tick, step, k, e_tick):
    """The comment block at the top of ekf_multirate.hpp, read literally: the history holds the entries first .. tick-1, the measurement
    belongs to the one `step` back (the oldest if there are fewer), and the chain restarts from the newest stored state in (first, mt]
    -- a grid checkpoint (every k-th tick) or the extra one (tick e_tick) -- or else from the anchor at `first`."""
    entries = list(range(first, tick))
    mt = entries[max(len(entries) - step, 0)]
    for t in range(mt, first, -1):
        if t % k == 0:                      # (the host never places the extra slot on a grid tick: the grid checkpoint serves)
            return mt, t, "grid"
        if t == e_tick:
            return mt, t, "extra"
    return mt, first, "anchor"


def age_for_step(s):
    """A measurement age whose dynamic step delay is s ticks, a fifth of a tick away from where the rounding would tip."""
    return s * DT + 0.001


def step_of_age(age, delay_max):
    return max(int(min(age + OFFSET, delay_max) / DT + 0.5), 1)


class HistoryModel:
    """Index bookkeeping of one multirate handle.  Ticks are the handle's (shifted) ticks, like the device's."""

    def __init__(self, B, k, step_max, upd_per_meas, rebase_at=1 << 30):
        self.B, self.k = B, k
        self.Nc, self.Cu = history_sizes(step_max, k)
        self.upd_per_meas = upd_per_meas
        self.rebase_at = rebase_at
        self.tick = 0
        self.origin = 0                       # ticks removed by origin shifts
        self.e_tick = self.e_want = self.last_launch = -1
        self.first = np.zeros(B, np.int64)
        self.seeded = np.zeros(B, bool)
        self.prepared = False
        # who wrote each lane's copy of a slot last: 0 nobody, 1 a predict launch or the current tick of k_step_mr, 2 a replay
        self.grid_w = np.zeros((self.Nc, B), np.int8)
        self.extra_w = np.zeros(B, np.int8)
        self.arm_shifted = self.fill_shifted = False
        self.e_fill_launch = -2               # last_launch at the time the extra slot was filled: "filled for this frame"
        self.counts = dict.fromkeys(CLASSES, 0)
        self.counts["E_long"] = 0
        self.log = []                         # (absolute tick, lane, class string) of every correcting lane-tick

    # ---- host side
    def seed(self, mask):
        if not self.prepared:                 # mr_prepare: every filter's history is the single entry "state now"
            self.first[:] = self.tick - 1
            self.e_tick = self.e_want = self.last_launch = -1
            self.prepared = True
        mask = np.asarray(mask, bool)
        self.first[mask] = self.tick - 1      # k_seed
        self.seeded |= mask

    def _advance(self):
        self.tick += 1
        if self.tick >= self.rebase_at:       # advance_tick
            shift = ((self.rebase_at // 2) // self.Cu) * self.Cu
            if shift <= 0:
                return
            self.first = np.maximum(self.first - shift, NEVER)
            self.tick -= shift
            if self.e_want >= 0:
                self.counts["La"] += 1
            if self.e_tick >= 0:
                self.fill_shifted = True
            for name in ("e_tick", "e_want", "last_launch"):
                v = getattr(self, name)
                if v >= 0:
                    setattr(self, name, max(v - shift, -1))
            if self.e_fill_launch >= 0:
                self.e_fill_launch = max(self.e_fill_launch - shift, -1)
            self.origin += shift

    def tick_predict(self):
        """A predict-only launch (k_predict with the history arguments of mr_ck_for_predict)."""
        t = self.tick
        if t % self.k == 0:
            if t == self.e_want:
                self.e_want = -1              # the grid checkpoint of this tick serves
            self.grid_w[(t // self.k) % self.Nc, :] = 1
        elif t == self.e_want:
            self.e_want = -1
            self.e_tick = t
            self.extra_w[:] = 1
            self.fill_shifted = False
            self.e_fill_launch = self.last_launch
        self._advance()

    def tick_step(self, corr, step, sched_step, per_filter_delays):
        """A launch of k_step_mr.  corr [B] bool: who performs a correction; step [B] or int: their step delays; sched_step: the step
        delay the host assumes for the next frame; per_filter_delays: dynamic delay with per-filter stamps."""
        n, k, e = self.tick, self.k, self.e_tick
        corr = np.asarray(corr, bool) & self.seeded
        step = np.broadcast_to(np.asarray(step), (self.B,))
        fresh_extra = e >= 0 and self.e_fill_launch == self.last_launch   # filled since the previous k_step_mr launch
        lanes = {}
        for i in np.nonzero(corr)[0]:
            first = int(self.first[i])
            mt, start, kind = choose_start(first, n, int(step[i]), k, e if e >= 0 else NEVER)
            lanes[int(i)] = (first, mt, start, kind)
        for w0 in range(0, self.B, WAVE):
            wl = range(w0, min(w0 + WAVE, self.B))
            early = all((not self.seeded[i]) or (i in lanes and lanes[i][2] == lanes[i][1]) for i in wl)
            for i in wl:
                if i not in lanes:
                    continue
                first, mt, start, kind = lanes[i]
                cls = []
                if kind == "extra":
                    pre = mt - start
                    cls.append(("D" if early else "H") if pre == 0 else ("E" if pre <= 2 else "E_long"))
                    if self.extra_w[i] == 2:
                        cls.append("Je")
                    if self.fill_shifted:
                        cls.append("Lu")
                else:
                    if kind == "anchor":
                        cls.append("A" if mt == first else "B")
                    else:
                        cls.append("C0" if mt % k == 0 else "C+")
                        slot = (start // k) % self.Nc
                        if self.grid_w[slot, i] == 2:
                            cls.append("Jg")
                        if (start + self.origin) // k >= self.Nc:
                            cls.append("Kg")
                    if fresh_extra:
                        if e > mt:
                            cls.append("F")
                        elif e <= start:
                            cls.append("G")
                if start + 1 <= n - 1 and floor_div(start + 1, self.Cu) != floor_div(n - 1, self.Cu):
                    cls.append("K")
                for c in cls:
                    self.counts[c] += 1
                self.log.append((n + self.origin, i, "+".join(cls)))
        # what the launch writes: the replays rewrite the checkpoints they pass, the current tick writes its own grid checkpoint
        for i, (first, mt, start, kind) in lanes.items():
            for t in range(mt + 1, n):
                if t % k == 0:
                    self.grid_w[(t // k) % self.Nc, i] = 2
                if t == e:
                    self.extra_w[i] = 2
            self.first[i] = mt
        if n % k == 0:
            self.grid_w[(n // k) % self.Nc, self.seeded] = 1
        # mr_schedule_extra
        period = n - self.last_launch if self.last_launch >= 0 else self.upd_per_meas
        self.last_launch = n
        ew = n + period - sched_step
        self.e_want = ew if (ew > n and period > 1 and period + sched_step < self.Cu and not per_filter_delays) else -1
        self._advance()


# ------------------------------------------------------------------------------------------------ schedules
MODES = ("fixed", "uniform", "stamps")
KS = (4, 8, 32)
T_MAX = 160
SEED_TICK = 1                       # one tick passes before the first filters are seeded: their history then starts at tick 0

# Gaps between frames (ticks) after the first frame at tick 3, per (k, mode): chosen on the CPU until the census of
# tests/test_multirate_schedule_cpu.py met its counts.  The cadence is p with a fixed jitter pattern; the short gaps put a frame
# inside the previous frame's replayed range, the long ones let a grid checkpoint pass between the extra slot and the entry.
GAPS = {   # (k, mode, rebase run)
    (4, "fixed", False): (3, 7, 6, 3, 3, 5, 8, 6, 6, 7, 7, 8, 5, 6, 6, 7, 3, 7, 8, 6, 4, 7, 6, 5, 6, 8),
    (8, "fixed", False): (3, 6, 6, 7, 6, 5, 8, 6, 6, 7, 6, 5, 8, 6, 6, 7, 6, 5, 8, 6, 6, 7, 6, 5, 8),
    (32, "fixed", False): (6, 6, 6, 6, 9, 5, 8, 6, 7, 7, 3, 4, 8, 8, 6, 9, 8, 7, 4, 3, 2, 7, 3, 6, 9),
    (4, "uniform", False): (3, 7, 6, 3, 6, 5, 8, 6, 7, 7, 7, 8, 8, 6, 3, 6, 3, 7, 8, 6, 2, 7, 6, 5, 6, 8),
    (8, "uniform", False): (3, 6, 6, 3, 3, 5, 8, 6, 7, 7, 6, 8, 5, 6, 6, 7, 3, 5, 8, 6, 6, 7, 6, 5, 6, 6, 6),
    (32, "uniform", False): (3, 8, 9, 7, 8, 3, 8, 6, 7, 7, 7, 8, 8, 6, 6, 6, 7, 5, 3, 6, 7, 6, 7, 6),
    (4, "stamps", False): (3, 6, 6, 7, 6, 5, 8, 6, 6, 7, 6, 5, 8, 6, 6, 7, 6, 5, 8, 6, 6, 7, 6, 5, 8),
    (8, "stamps", False): (3, 6, 6, 7, 6, 5, 8, 6, 6, 7, 6, 5, 8, 6, 6, 7, 6, 5, 8, 6, 6, 7, 6, 5, 8),
    (32, "stamps", False): (3, 6, 6, 7, 6, 5, 8, 6, 6, 7, 6, 5, 5, 6, 6, 7, 6, 5, 8, 6, 6, 7, 6, 5, 6, 6),
    (4, "fixed", True): (3, 6, 6, 3, 6, 5, 8, 3, 6, 7, 7, 5, 5, 6, 3, 6, 3, 3, 8, 6, 2, 7, 6, 5, 6, 8, 8, 3, 3),
}
RUNS = [(k, mode, False) for mode in ("fixed", "uniform", "stamps") for k in (4, 8, 32)] + [(4, "fixed", True)]
# Step delays per frame for the uniform-age mode (age_for_step), cycled.
STEPS_UNIFORM = (3, 3, 3, 4, 4, 3, 2, 2, 3, 5, 5, 3)
STEPS_STAMPS = (2, 3, 4, 5)


def params_kw(mode):
    kw = dict(update_freq=100.0, direct_orien_method=1, multirate_ekf=1, corner_margin_enbl=1, limit_measurement_freq=0,
              measurement_delay=0.030)
    if mode == "fixed":
        kw.update(dynamic_meas_delay=0)
    else:
        kw.update(dynamic_meas_delay=1, measurement_delay_max=0.050, dyn_measurement_delay_offset=OFFSET)
    return kw


def step_max_of(mode):
    return 3 if mode == "fixed" else 5


class Schedule:
    """Frame ticks, per-frame lane masks, seeding ticks and measurement ages of one (k, mode) run."""

    def __init__(self, k, mode, gaps=None, rebase=False):
        self.k, self.mode, self.B = k, mode, B_SCHED
        self.kw = params_kw(mode)
        self.step_max = step_max_of(mode)
        self.Nc, self.Cu = history_sizes(self.step_max, k)
        self.rebase_at = 4 * self.Cu if rebase else 1 << 30
        gaps = list(GAPS[(k, mode, rebase)] if gaps is None else gaps)
        ticks, t = [], 3
        for g in [0] + gaps:
            t += g
            if t >= T_MAX:
                break
            ticks.append(t)
        self.frame_ticks = ticks
        self.T = min(T_MAX, ticks[-1] + 2)
        nf, B = len(ticks), self.B
        rng = np.random.default_rng(1000 * k + MODES.index(mode))
        mask = np.ones((nf, B), bool)
        self.late = np.arange(64, 76)            # seeded on their own first detection, a few frames in
        self.alternate = np.arange(76, 88)       # masked on alternate frames
        self.never = np.arange(88, 96)           # never see a tag
        first_frame = np.zeros(B, np.int64)
        first_frame[self.late] = 3 + (np.arange(len(self.late)) * 5) % max(nf - 6, 1)
        first_frame[self.never] = nf
        for f in range(nf):
            mask[f, self.alternate] = (f + self.alternate) % 2 == 0
            mask[f, first_frame > f] = False
        mask[:, 128:] &= rng.uniform(size=(nf, B - 128)) < 0.55   # wave 2: every lane its own frames, so the anchors differ in age
        mask[:2, 128:] = True                                      # the clamped and the first anchor start reach wave 2 as well
        self.mask = mask
        self.seed_tick = np.full(B, SEED_TICK, np.int64)
        self.seed_tick[self.late] = np.array(ticks)[first_frame[self.late]]
        self.seed_tick[self.never] = -1
        # step delays: per frame (uniform age) or per frame and lane (stamps)
        if mode == "fixed":
            self.steps = np.full((nf, B), 3)
        elif mode == "uniform":
            self.steps = np.array([STEPS_UNIFORM[f % len(STEPS_UNIFORM)] for f in range(nf)])[:, None].repeat(B, 1)
        else:
            self.steps = np.array(STEPS_STAMPS)[rng.integers(0, len(STEPS_STAMPS), size=(nf, B))]
        self.ages = age_for_step(self.steps.astype(np.float64))
        self.upd_per_meas = None

    def model(self, upd_per_meas):
        return HistoryModel(self.B, self.k, self.step_max, upd_per_meas, self.rebase_at)

    def frame_of(self, t):
        return self.frame_ticks.index(t) if t in self.frame_ticks else None


def run_model(sched, perf_of=None, upd_per_meas=4):
    """The model over a schedule with corrections = the frame masks of the seeded filters (no oracle: what the schedule search uses),
    or perf_of(t) [B] bool when given."""
    m = sched.model(upd_per_meas)
    m.seed(np.zeros(sched.B, bool))
    for t in range(sched.T):
        m.seed(sched.seed_tick == t) if (sched.seed_tick == t).any() else None
        f = sched.frame_of(t)
        if f is None:
            m.tick_predict()
        else:
            corr = sched.mask[f] if perf_of is None else perf_of(t)
            m.tick_step(corr, sched.steps[f], int(sched.steps[f, 0]) if sched.mode != "fixed" else 3, sched.mode == "stamps")
    return m


REQUIRED = {"fixed": ("A", "B", "C0", "C+", "D", "E", "F", "G", "H", "Jg", "Je", "K", "Kg"),
            "uniform": ("A", "B", "C0", "C+", "D", "E", "F", "G", "H", "Jg", "Je", "K", "Kg"),
            "stamps": ("A", "B", "C0", "C+", "Jg", "K", "Kg")}
EMPTY_WITH_STAMPS = ("D", "E", "E_long", "F", "G", "H", "Je")
MIN_COUNT = 8


# ------------------------------------------------------------------------------------------------ driving a schedule
class _Views:
    """numpy views of one oracle filter's state (no copies: the arrays live inside the ctypes struct)."""

    def __init__(self, filt):
        f = filt.f
        self.parts = [np.frombuffer(a, dtype=np.float64) for a in (f.r_nom, f.v_nom, f.q_nom, f.ab_nom, f.wb_nom)]
        self.cov = np.frombuffer(f.cov_pert, dtype=np.float64)

    def x(self):
        return np.concatenate(self.parts)


def run_schedule(sched, oracle, po, meas_near, dtype="f64", ekf=None, after_tick=None):
    """Step one oracle.Filter per filter (and the engine handle `ekf`, when given) through a schedule, the model beside them, driven
    by the oracle's performed_correction.  Inputs come from the oracle's states alone, so every run of a schedule sees the same
    IMU samples and tag poses whatever it compares them with: a gentle hover (the fp32 free run stays comparable tick by tick) and
    tag poses near the state.  after_tick(t, ctx) is called after every tick.  Returns the model."""
    B, n = sched.B, po.num_states
    rng = np.random.default_rng(4242 + sched.k)
    rnd = (lambda a: a.astype(np.float32).astype(np.float64)) if dtype == "f32" else (lambda a: a)
    filt = [oracle.Filter(po) for _ in range(B)]
    views = [_Views(f) for f in filt]
    model = sched.model(int(po.upd_per_meas))
    seeded = np.zeros(B, bool)
    z0 = np.zeros((B, 7))
    z0[:, 0:2] = rng.normal(size=(B, 2)) * 0.1; z0[:, 2] = rng.uniform(0.8, 2.0, size=B)
    z0[:, 3:7] = np.array([0.7071067811865476, -0.7071067811865476, 0.0, 0.0])
    z0 = rnd(z0)
    model.seed(np.zeros(B, bool))
    if ekf is not None:
        ekf.enable_gating(True)
        ekf.initialize_state(z0, reinit_bias=True, mask=np.zeros(B, np.uint8))   # nothing seeded yet: the handle just accepts ticks
    xr = np.zeros((B, 16)); Pr = np.zeros((B, n, n))
    for t in range(sched.T):
        tc = DT * t
        u = np.zeros((B, 6))
        u[:, 0:3] = np.array([0.0, 0.0, 9.81]) + rng.normal(size=(B, 3)) * 0.05
        u[:, 3:6] = rng.normal(size=(B, 3)) * 0.02
        u = rnd(u)
        f = sched.frame_of(t)
        seed_now = sched.seed_tick == t
        mask = sched.mask[f].copy() if f is not None else np.zeros(B, bool)
        z = None
        if f is not None:
            guess = xr.copy()
            guess[~seeded, 6:10] = np.array([0.0, 0.0, 0.0, 1.0])
            z = rnd(meas_near(rng, po, guess, ang=0.05, pos=0.02))
            z[seed_now] = z0[seed_now]                       # a filter's first detection seeds it and is its first measurement
        stamp = tc - sched.ages[f] if f is not None else np.zeros(B)
        for i in np.nonzero(seed_now)[0]:
            filt[i].set_apriltag(z0[i, :3], z0[i, 3:], stamp[i])   # seeds the oracle filter (NODE.cpp:169-174)
            filt[i].f.measurement_ready = 0
        if seed_now.any():
            model.seed(seed_now)
            if ekf is not None:
                ekf.initialize_state(z0, reinit_bias=True, mask=seed_now.astype(np.uint8))
                if dtype == "f32":   # start the oracle's copy of a freshly seeded filter from the engine's fp32-rounded state
                    xs = ekf.get_state()[0]
                    for i in np.nonzero(seed_now)[0]:
                        fi = filt[i].f
                        for k in range(3):
                            fi.r_nom[k] = xs[i, k]; fi.v_nom[k] = xs[i, 3 + k]; fi.ab_nom[k] = xs[i, 10 + k]; fi.wb_nom[k] = xs[i, 13 + k]
                        for k in range(4):
                            fi.q_nom[k] = xs[i, 6 + k]
                        for k in range(16):
                            fi.x_hist[k] = xs[i, k]
            seeded |= seed_now
        for i in range(B):
            filt[i].set_imu(u[i, :3], u[i, 3:])
            if mask[i]:
                filt[i].set_apriltag(z[i, :3], z[i, 3:], stamp[i])
            filt[i].filter_update(tc)
        perf = np.array([fl.f.performed_correction for fl in filt], bool) & seeded
        if ekf is not None:
            m8 = mask.astype(np.uint8)
            if sched.mode == "fixed":
                ekf.filter_update(u, z, m8 if z is not None else None)
            elif sched.mode == "uniform":
                if f is not None:
                    ekf.set_uniform_measurement_age(float(sched.ages[f, 0]))
                ekf.filter_update(u, z, m8 if z is not None else None, t_curr=tc)
            else:
                ekf.filter_update(u, z, m8 if z is not None else None, t_curr=tc, apriltag_time=stamp if z is not None else None)
        if f is None:
            model.tick_predict()
        else:
            model.tick_step(perf, sched.steps[f], int(sched.steps[f, 0]) if sched.mode != "fixed" else int(po.measurement_step_delay),
                            sched.mode == "stamps")
        for i in np.nonzero(seeded)[0]:
            xr[i] = views[i].x(); Pr[i] = views[i].cov[: n * n].reshape(n, n)
        if after_tick is not None:
            after_tick(t, dict(filt=filt, model=model, seeded=seeded, perf=perf, mask=mask, frame=f, xr=xr, Pr=Pr, stamp=stamp))
    return model


def census_ok(sched, counts):
    """The counts a run of this schedule must reach (conditions, not measurements); returns the list of classes that fall short."""
    short = [c for c in REQUIRED[sched.mode] if counts[c] < MIN_COUNT]
    if sched.mode == "stamps":
        short += [c for c in EMPTY_WITH_STAMPS if counts[c] != 0]
    if sched.rebase_at < (1 << 30):
        short += [c for c in ("La", "Lu") if counts[c] < 1]
    return short
