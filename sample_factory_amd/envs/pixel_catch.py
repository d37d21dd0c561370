"""PixelCatch: a small, deterministic, learnable pixel game.  A ball falls down an H x W field and reflects
off the side walls; the player moves a paddle along the bottom rows and is paid +1 for a ball it catches, -1 for one it
misses.  An episode is `balls` balls.  The observation is k history planes of the field, u8: background 0, paddle 128, ball
255; only from the difference between planes can the policy tell where the ball is heading.

This module holds the game three times:
  * the MODEL, in NumPy, integer arithmetic only (`geometry`, `philox`, `draw_ball`, `model_reset`, `model_step`, `render`,
    `episode_level`, `level_decoys`, `oracle_action`).  It is the contract: the kernel (csrc/sf_pixcatch.hip) equals it bit for bit, as envs/frame_ops.py is
    the contract of the resize kernel;
  * `PixelCatchVecEnv`, the device env: state in a device tensor, ONE launch per step that also renders the next
    observation straight into slot t + 1 of the trajectory slab (`reset_into` / `step_into`, the zero-copy hooks the runner
    detects), next to gymnasium-style `reset` / `step`;
  * `PixelCatchHostEnv`, the model as a host vector env returning numpy arrays (inline or in env worker processes; with
    frames=1 under --device_framestack=k it is the same task through the host-env ingest path).

Constants (`geometry(H, W)`, all integer; m = min(H, W)):
    ball            bs x bs,  bs = max(2, m // 21)                       84 x 84: 4 x 4     36 x 36: 2 x 2
    paddle          pw x ph,  pw = max(3, W // 7), ph = max(1, H // 28)           12 x 3             5 x 1
    paddle speed    ps = ceil(W / 28) pixels per step                             3                  2
    ball speed      |vx| <= vxm = max(1, W // 42);  vy in 1 .. vym                vxm 2, vym 2       vxm 1, vym 2
    landing row     the ball has reached the paddle's rows when by >= D = H - ph - bs + 1
    vym             2 if ceil(D / 2) * ps >= W - pw else 1: the paddle crosses the whole field while the fastest ball falls
A field is valid when D >= 2, W - pw >= 1, W - bs >= vxm (one reflection per step), D * ps >= W - pw and H, W <= 1024.

State of one env: int32 [4 + 3 k] = {draw index, balls left, vx, vy}, then per plane j {paddle x, ball x, ball y}; plane
k - 1 is the current position, plane j the one k - 1 - j steps ago (the order gym.wrappers.FrameStack produces).

Step: the paddle moves (action 0 stay, 1 left, 2 right, anything else stay) and is clamped; the ball moves by (vx, vy) and
reflects off the side walls; if by >= D the reward is +1 when the column ranges [px, px + pw) and [bx, bx + bs) overlap, else
-1, balls left drops by one and a new ball is drawn at the top (row 0): column, vx, vy from ONE Philox4x32-10 block, counter
(draw index, 0, 4, 0), key (seed, global env id), each reduced by multiply-high.  After the last ball terminated = 1 and the
env resets itself in the same step: paddle centred, new ball, every plane shows the new first frame.  A new ball inside an
episode leaves the older planes alone.  truncated is always 0.

Levels (`decoys` nd in 0 .. 8, `levels` L >= 0, `start_level` S; nd = 0 is the game above bit for bit).  A level places nd
static decoys in the field: squares that look exactly like the ball and never move.  Levels change the rendered frame
only: state words, rewards and flags are those of the game without decoys for the same actions.
    episode     ep = (state[0] - 1) // balls: the draw index counts the balls drawn, `balls` of them per episode
    its level   w = philox(counter (ep, 0, 6, 0), key (seed, global env id));  level = (S + mulhi(w[0], L)) mod 2^32 for a
                finite set of L > 0 levels, (S + w[0]) mod 2^32 for L = 0 (unlimited levels, Procgen's convention)
    decoy d     w = philox(counter (d, 0, 7, 0), key (LEVEL_KEY, level)): the bs x bs square at x = mulhi(w[0], W - bs + 1),
                y = mulhi(w[1], D).  Its rows end at H - ph - 1 at the latest: a decoy never touches the paddle's rows.  The
                key holds neither the run's seed nor the env: level 7 looks the same in every run.
A pixel is 255 if it lies in the ball or in a decoy, else 128 if it lies in the paddle, else 0.  All k planes show the
decoys of the current episode's level.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from sample_factory_amd.envs import spaces

Geometry = namedtuple("Geometry", "bs pw ph ps vxm vym D")
HDR, MAX_FRAMES, MAX_SIDE = 4, 8, 1024
BACKGROUND, PADDLE, BALL = 0, 128, 255
MAX_DECOYS, LEVEL_KEY = 8, 0x4C564C53
DEVICE_MAX_DECOY_PIXELS = 65516  # sf_pixcatch_*_levels: H W + 20 bytes of LDS per work-group, 64 KB at the most
_M32 = np.uint64(0xFFFFFFFF)


def geometry(H: int, W: int) -> Geometry:
    H, W = int(H), int(W)
    m = min(H, W)
    bs, pw, ph = max(2, m // 21), max(3, W // 7), max(1, H // 28)
    ps, vxm = (W + 27) // 28, max(1, W // 42)
    D = H - ph - bs + 1
    vym = 2 if ((D + 1) // 2) * ps >= W - pw else 1
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE and D >= 2 and W - pw >= 1 and W - bs >= vxm and D * ps >= W - pw):
        raise ValueError(f"PixelCatch: a {H} x {W} field is too small (or above {MAX_SIDE}) for ball and paddle")
    return Geometry(bs, pw, ph, ps, vxm, vym, D)


def state_words(k: int) -> int:
    if not 1 <= int(k) <= MAX_FRAMES:
        raise ValueError(f"PixelCatch: frames = {k} outside 1 .. {MAX_FRAMES}")
    return HDR + 3 * int(k)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) over numpy arrays / scalars: the words of sf_philox4x32_10, as 4 uint32 arrays"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(x, dtype=np.uint64) & _M32 for x in (c0, c1, c2, c3, k0, k1)))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def _mulhi(word, n: int):
    return ((word.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int32)


def draw_ball(draw, env_ids, seed: int, g: Geometry, W: int):
    """the ball of draw index `draw` (int32 [n]) of the envs `env_ids`: (bx, vx, vy) int32 [n]; by is 0"""
    w = philox(draw.astype(np.uint32), 0, 4, 0, int(seed) & 0xFFFFFFFF, np.asarray(env_ids).astype(np.uint32))
    return _mulhi(w[0], W - g.bs + 1), _mulhi(w[1], 2 * g.vxm + 1) - np.int32(g.vxm), np.int32(1) + _mulhi(w[2], g.vym)


def check_levels(decoys: int, levels: int, start_level: int):
    """(nd, L, S) as ints, or ValueError"""
    nd, L, S = int(decoys), int(levels), int(start_level)
    if not 0 <= nd <= MAX_DECOYS:
        raise ValueError(f"PixelCatch: decoys = {nd} outside 0 .. {MAX_DECOYS}")
    if L < 0 or L > 0x7FFFFFFF:
        raise ValueError(f"PixelCatch: levels = {L} must be 0 (unlimited) .. 2^31 - 1")
    if not 0 <= S <= 0xFFFFFFFF:
        raise ValueError(f"PixelCatch: start_level = {S} is no uint32")
    return nd, L, S


def episode_level(state: np.ndarray, env_ids, seed: int, balls: int, levels: int = 0, start_level: int = 0) -> np.ndarray:
    """the level id (uint32 [N]) of the episode each env is in, from the state after a reset or a step"""
    _, L, S = check_levels(0, levels, start_level)
    ep = (state[:, 0].astype(np.int64) - 1) // int(balls)
    w = philox(ep.astype(np.uint32), 0, 6, 0, int(seed) & 0xFFFFFFFF, np.asarray(env_ids).astype(np.uint32))
    off = ((w[0].astype(np.uint64) * np.uint64(L)) >> np.uint64(32)) if L > 0 else w[0].astype(np.uint64)
    return ((np.uint64(S) + off) & _M32).astype(np.uint32)


def level_decoys(level, nd: int, H: int, W: int):
    """the decoys of `level` (uint32 scalar or [N]): (x, y) int32 [..., nd], top-left corners of bs x bs squares"""
    g = geometry(H, W)
    nd = check_levels(nd, 0, 0)[0]
    w = philox(np.arange(nd, dtype=np.uint32), 0, 7, 0, LEVEL_KEY, np.asarray(level).astype(np.uint32)[..., None])
    return _mulhi(w[0], W - g.bs + 1), _mulhi(w[1], g.D)


def model_reset(N: int, env0: int, seed: int, H: int, W: int, k: int, balls: int, decoys: int = 0, levels: int = 0,
                start_level: int = 0) -> np.ndarray:
    """first state int32 [N, 4 + 3 k] of envs [env0, env0 + N); levels change frames only (the arguments are checked)"""
    check_levels(decoys, levels, start_level)
    g = geometry(H, W)
    st = np.zeros((int(N), state_words(k)), np.int32)
    bx, vx, vy = draw_ball(st[:, 0], env0 + np.arange(N), seed, g, W)
    st[:, 0], st[:, 1], st[:, 2], st[:, 3] = 1, int(balls), vx, vy
    st[:, HDR::3], st[:, HDR + 1::3], st[:, HDR + 2::3] = (W - g.pw) // 2, bx[:, None], 0
    return st


def model_step(state: np.ndarray, actions, env0: int, seed: int, H: int, W: int, k: int, balls: int, decoys: int = 0,
               levels: int = 0, start_level: int = 0):
    """one step of every env: (new state, rewards f32 [N], terminated bool [N]); `state` is left unchanged.  Levels change
    frames only (the arguments are checked)"""
    check_levels(decoys, levels, start_level)
    g = geometry(H, W)
    st = state.copy()
    N, c = st.shape[0], HDR + 3 * (int(k) - 1)
    a = np.asarray(actions).reshape(-1).astype(np.int64)
    px, bx, by, vx, vy = st[:, c].copy(), st[:, c + 1].copy(), st[:, c + 2].copy(), st[:, 2].copy(), st[:, 3].copy()
    px = np.clip(px + np.where(a == 1, -g.ps, np.where(a == 2, g.ps, 0)).astype(np.int32), 0, W - g.pw).astype(np.int32)
    bx = bx + vx
    lo = bx < 0
    bx, vx = np.where(lo, -bx, bx), np.where(lo, -vx, vx)
    hi = bx > W - g.bs
    bx, vx = np.where(hi, 2 * (W - g.bs) - bx, bx), np.where(hi, -vx, vx)
    by = by + vy
    landed = by >= g.D
    caught = (px < bx + g.bs) & (bx < px + g.pw)
    rewards = np.where(landed, np.where(caught, 1.0, -1.0), 0.0).astype(np.float32)
    left = st[:, 1] - landed
    term = landed & (left == 0)
    left = np.where(term, int(balls), left)
    px = np.where(term, (W - g.pw) // 2, px)
    at = np.flatnonzero(landed)
    if at.size:  # a new ball at the top for those that landed
        bx[at], vx[at], vy[at] = draw_ball(st[at, 0], env0 + at, seed, g, W)
        by[at] = 0
    st[:, 0] += landed
    st[:, 1], st[:, 2], st[:, 3] = left, vx, vy
    st[:, HDR:c] = state[:, HDR + 3:]  # the history moves up one plane ...
    st[:, c], st[:, c + 1], st[:, c + 2] = px, bx, by
    st[term, HDR:] = np.tile(st[term, c:c + 3], (1, int(k)))  # ... or, at an episode's end, shows the first frame k times
    return st, rewards, term


def render(state: np.ndarray, H: int, W: int, k: int, env0: int = 0, seed: int = 0, balls: int = 1, decoys: int = 0,
           levels: int = 0, start_level: int = 0) -> np.ndarray:
    """the observation u8 [N, k, H, W] of `state`: rectangles painted from the state words, paddle first, ball and the
    decoys of the episode's level over it (env0, seed and balls matter only with decoys > 0)"""
    g = geometry(H, W)
    N = state.shape[0]
    nd = check_levels(decoys, levels, start_level)[0]
    obs = np.zeros((N, int(k), H, W), np.uint8)
    n = np.arange(N)[:, None, None]
    for j in range(int(k)):
        px, bx, by = (state[:, HDR + 3 * j + i].astype(np.int64)[:, None, None] for i in range(3))
        obs[n, j, (H - g.ph) + np.arange(g.ph)[None, :, None], px + np.arange(g.pw)[None, None, :]] = PADDLE
        obs[n, j, by + np.arange(g.bs)[None, :, None], bx + np.arange(g.bs)[None, None, :]] = BALL
    if nd:
        level = episode_level(state, int(env0) + np.arange(N), seed, balls, levels, start_level)
        dx, dy = (c.astype(np.int64) for c in level_decoys(level, nd, H, W))
        for d in range(nd):
            rows, cols = dy[:, d, None, None] + np.arange(g.bs)[None, :, None], dx[:, d, None, None] + np.arange(g.bs)[None, None, :]
            for j in range(int(k)):
                obs[n, j, rows, cols] = BALL
    return obs


def landing_column(state: np.ndarray, H: int, W: int, k: int) -> np.ndarray:
    """ball x at the step the current ball reaches the paddle's rows, side-wall bounces included: int32 [N]"""
    g = geometry(H, W)
    c = HDR + 3 * (int(k) - 1)
    bx, by, vx, vy = (state[:, i].astype(np.int64) for i in (c + 1, c + 2, 2, 3))
    steps = (g.D - by + vy - 1) // vy
    span = W - g.bs                              # bx walks a triangle wave of period 2 span over [0, span]
    z = np.mod(bx + vx * steps, 2 * span)
    return np.where(z > span, 2 * span - z, z).astype(np.int32)


def oracle_action(state: np.ndarray, H: int = 84, W: int = 84, k: int = 4) -> np.ndarray:
    """the player who knows the landing column: moves the paddle's centre towards the ball's centre at landing"""
    g = geometry(H, W)
    px = state[:, HDR + 3 * (int(k) - 1)].astype(np.int64)
    target = np.clip(landing_column(state, H, W, k) + g.bs // 2 - g.pw // 2, 0, W - g.pw)
    diff = target - px
    return np.where(2 * diff > g.ps, 2, np.where(2 * diff < -g.ps, 1, 0)).astype(np.int32)


def _spaces(H, W, k):
    return spaces.Dict({"obs": spaces.Box(0, 255, (int(k), int(H), int(W)), np.uint8)}), spaces.Discrete(3)


class PixelCatchHostEnv:
    """the NumPy model as a host vector env: numpy in, numpy out (what envpool-style envs hand over)"""

    def __init__(self, num_agents=64, size=(84, 84), frames=4, balls_per_episode=4, seed=0, env0=0, decoys=0, levels=0,
                 start_level=0):
        self.num_agents, (self.H, self.W), self.k = int(num_agents), (int(size[0]), int(size[1])), int(frames)
        self.balls, self.seed_, self.env0 = int(balls_per_episode), int(seed), int(env0)
        self.decoys, self.levels, self.start_level = check_levels(decoys, levels, start_level)
        geometry(self.H, self.W), state_words(self.k)
        self.observation_space, self.action_space = _spaces(self.H, self.W, self.k)
        self.state = None

    def _render(self):
        return render(self.state, self.H, self.W, self.k, self.env0, self.seed_, self.balls, self.decoys, self.levels,
                      self.start_level)

    def reset(self, **kwargs):
        self.state = model_reset(self.num_agents, self.env0, self.seed_, self.H, self.W, self.k, self.balls)
        return {"obs": self._render()}, {}

    def step(self, actions):
        if self.state is None:
            self.reset()
        self.state, rew, term = model_step(self.state, actions, self.env0, self.seed_, self.H, self.W, self.k, self.balls)
        return {"obs": self._render()}, rew, term, np.zeros(self.num_agents, np.bool_), {}

    def current_levels(self) -> np.ndarray:
        """level ids (uint32 [num_agents]) of the running episodes; for tests and logging"""
        if self.state is None:
            self.reset()
        return episode_level(self.state, self.env0 + np.arange(self.num_agents), self.seed_, self.balls, self.levels,
                             self.start_level)

    def close(self):
        pass


class PixelCatchVecEnv:
    """the device env (the reference's brax / isaacgym pattern: num_agents = N, tensors on the device, auto-reset) with
    the zero-copy hooks of SyntheticVecEnv: sf_pixcatch_step renders into obs_out = slab obs[:, t + 1]"""

    def __init__(self, num_agents=4096, size=(84, 84), frames=4, balls_per_episode=4, seed=0, env0=0, device="cuda",
                 decoys=0, levels=0, start_level=0):
        import torch

        from sample_factory_amd import lib
        self._lib = lib
        self.num_agents, (self.H, self.W), self.k = int(num_agents), (int(size[0]), int(size[1])), int(frames)
        self.balls, self.seed_, self.env0 = int(balls_per_episode), int(seed), int(env0)
        self.decoys, self.levels, self.start_level = check_levels(decoys, levels, start_level)
        geometry(self.H, self.W)
        if self.decoys and self.H * self.W > DEVICE_MAX_DECOY_PIXELS:
            raise ValueError(f"PixelCatch: the device env keeps a plane of decoys in LDS, {self.H} x {self.W} is above "
                             f"{DEVICE_MAX_DECOY_PIXELS} pixels (PixelCatchHostEnv has no such limit)")
        self.obs_shape = (self.k, self.H, self.W)
        self.observation_space, self.action_space = _spaces(self.H, self.W, self.k)
        self.device = torch.device(device)
        self.state = torch.zeros((self.num_agents, state_words(self.k)), dtype=torch.int32, device=self.device)
        self._rew = torch.zeros(self.num_agents, dtype=torch.float32, device=self.device)
        self._term = torch.zeros(self.num_agents, dtype=torch.bool, device=self.device)
        self._trunc = torch.zeros(self.num_agents, dtype=torch.bool, device=self.device)
        self._obs = None
        self._started = False

    # -- zero-copy interface used by the native rollout runner
    def reset_into(self, obs_out) -> None:
        """obs_out: [N, k, H, W] u8 view (possibly strided over dim 0, e.g. slab[:, 0])"""
        if self.decoys:
            self._lib.pixcatch_reset_levels(self.state, obs_out, self.env0, self.seed_, self.balls, self.decoys, self.levels,
                                            self.start_level)
        else:
            self._lib.pixcatch_reset(self.state, obs_out, self.env0, self.seed_, self.balls)
        self._started = True

    def step_into(self, actions, obs_out):
        """actions int32 [N] on the device.  Returns (rewards f32, terminated bool, truncated bool) device tensors."""
        if self.decoys:
            self._lib.pixcatch_step_levels(self.state, actions, obs_out, self._rew, self._term, self.env0, self.seed_,
                                           self.balls, self.decoys, self.levels, self.start_level)
        else:
            self._lib.pixcatch_step(self.state, actions, obs_out, self._rew, self._term, self.env0, self.seed_, self.balls)
        return self._rew, self._term, self._trunc

    def current_levels(self) -> np.ndarray:
        """level ids (uint32 [num_agents]) of the running episodes, from the state words copied back; for tests and
        logging, not on the step path"""
        if not self._started:
            self.reset()
        return episode_level(self.state.cpu().numpy(), self.env0 + np.arange(self.num_agents), self.seed_, self.balls,
                             self.levels, self.start_level)

    # -- gymnasium-style interface (what a stock Sample Factory runner and enjoy call)
    def reset(self, **kwargs):
        import torch
        if self._obs is None:
            self._obs = torch.empty((self.num_agents,) + self.obs_shape, dtype=torch.uint8, device=self.device)
        self.reset_into(self._obs)
        return {"obs": self._obs}, {}

    def step(self, actions):
        import torch
        if not self._started or self._obs is None:
            self.reset()
        a = torch.as_tensor(actions, device=self.device).to(torch.int32).reshape(-1).contiguous()
        rew, term, trunc = self.step_into(a, self._obs)
        return {"obs": self._obs}, rew, term, trunc, {}

    def close(self):
        pass


def _args(cfg, env_config, default_agents):
    g = lambda name, d: (getattr(cfg, name, None) or d) if cfg is not None else d  # noqa: E731
    n, size = int(g("pixel_catch_agents", default_agents)), g("pixel_catch_size", 84)
    size = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
    # instance i of a multi-instance run simulates ids [env0 + i n, env0 + (i + 1) n), as make_synthetic_env does: the
    # union over instances is one instance with all the agents
    env0 = int(g("pixel_catch_env0", 0)) + int(getattr(env_config, "env_id", 0) or 0) * n
    return dict(num_agents=n, size=size, frames=int(g("pixel_catch_frames", 4)),
                balls_per_episode=int(g("pixel_catch_balls", 4)), seed=int(g("seed", 0)), env0=env0,
                decoys=int(g("pixel_catch_decoys", 0)), levels=int(g("pixel_catch_levels", 0)),
                start_level=int(g("pixel_catch_start_level", 0)))


def make_pixel_catch_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    """cfg.pixel_catch_agents / _size / _frames / _balls size the device env; _decoys / _levels / _start_level pick its levels"""
    return PixelCatchVecEnv(**_args(cfg, env_config, 4096))


def make_pixel_catch_host_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    """the same game on the host (numpy): --pixel_catch_frames=1 with --device_framestack=k stacks on the device"""
    return PixelCatchHostEnv(**_args(cfg, env_config, 64))


def add_pixel_catch_args(parser) -> None:
    parser.add_argument("--pixel_catch_agents", type=int, default=1024, help="games per env instance")
    parser.add_argument("--pixel_catch_size", type=int, default=84, help="the field is size x size pixels")
    parser.add_argument("--pixel_catch_frames", type=int, default=4, help="history planes per observation, 1 .. 8")
    parser.add_argument("--pixel_catch_balls", type=int, default=4, help="balls per episode")
    parser.add_argument("--pixel_catch_decoys", type=int, default=0, help="static decoy balls per level, 0 .. 8 (0: no levels)")
    parser.add_argument("--pixel_catch_levels", type=int, default=0, help="size of the level set; 0: unlimited levels")
    parser.add_argument("--pixel_catch_start_level", type=int, default=0, help="first level id of the set (uint32)")
