"""What a RaySensor observer costs (include/moog_engine.h moog_engine_add_sensor) and what it replaces:
colliding_predators_32 and falling_balls_64 at 4096 envs on an engine whose only observer is one sensor of 32 or 128 rays --
the HIP-event time of MOOG_K_TABLES per call (the sensor launch: the engine has no table) beside the step kernel's of the
same run -- and, on the same visit, the same tensor computed by a batched torch formulation from `env.field()` views and the
records' vertices, as a caller would write it without the observer ([envs, rays, edges] intermediates).

    python tools/bench_ray_sensor.py [--envs 4096] [--steps 100] [--out profiles/ray_sensor.txt]"""
import argparse
import os
import sys
import time


sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'moog.github.io_amd'))

WORKLOADS = ('colliding_predators_32', 'falling_balls_64')
RAYS = (32, 128)
MAX_RANGE = 2.0


def origin_layer(name):
    from moog import _compiler
    from moog_demos import example_configs
    c = _compiler.compile_config(layer_capacity=example_configs.capacity(name), **example_configs.load(name))
    return [k for k in c.layer_names if c.layer_slots[k][1] > 0][-1]


def config(name, rays):
    from moog import observers
    from moog_demos import example_configs
    cfg = example_configs.load(name)
    cfg['observers'] = {'rays': observers.RaySensor(origin_layer(name), num_rays=rays, max_range=MAX_RANGE)}
    return cfg


class TorchSensor(object):
    """The sensor 'rays' of `env` from field() views and the records' vertex words, in torch."""

    def __init__(self, env, torch):
        c = env.compiled
        P, L = c.program, c.layout
        T = dict(c.sensors)['rays']
        self.torch, self.env, self.T = torch, env, T
        dev = env.device
        slots = [T.row_slot[r] for r in range(T.n_rows) if T.row_slot[r] != T.origin_slot]
        row_of = {T.row_slot[r]: r for r in range(T.n_rows)}
        slot, v, first = [], [], []
        for s in slots:
            for k in range(P.slot_vcap[s]):
                slot.append(s)
                v.append(k)
                first.append(L.o_verts + 2 * P.slot_voff[s])
        self.slot = torch.tensor(slot, device=dev)
        self.v = torch.tensor(v, device=dev)
        self.first = torch.tensor(first, device=dev)
        self.row = torch.tensor([row_of[s] for s in slot], device=dev)
        self.d = torch.tensor(env.ray_directions('rays'), device=dev)
        self.origin = T.origin_slot

    def __call__(self, chunk=512):
        """[envs, rays, 2] float32, computed `chunk` envs at a time (the intermediates are [chunk, rays, edges] float64)."""
        n = self.env.num_envs
        return self.torch.cat([self.part(lo, min(n, lo + chunk)) for lo in range(0, n, chunk)])

    def part(self, lo, hi):
        torch, env = self.torch, self.env
        f = env.state_f64[lo:hi]
        n = env.state_i32[lo:hi, env.layout.o_nverts + self.slot]
        alive, opacity, pos = env.field('alive')[lo:hi], env.field('opacity')[lo:hi], env.field('position')[lo:hi]
        live = alive[:, self.slot].bool() & (opacity[:, self.slot] > 0) & (self.v < n) & (n >= 2)
        w = torch.where(self.v + 1 < n, self.v + 1, torch.zeros_like(n))
        ia, ib = (self.first + 2 * self.v).expand(hi - lo, -1), self.first + 2 * w
        ax, ay = f.gather(1, ia), f.gather(1, ia + 1)
        bx, by = f.gather(1, ib), f.gather(1, ib + 1)
        o = pos[:, self.origin]
        wx, wy, ex, ey = (ax - o[:, 0:1])[:, None], (ay - o[:, 1:2])[:, None], (bx - ax)[:, None], (by - ay)[:, None]
        dx, dy = self.d[None, :, 0:1], self.d[None, :, 1:2]
        den = dx * ey - dy * ex
        nt = wx * ey - wy * ex
        nu = wx * dy - wy * dx
        sg = torch.sign(den)
        t = nt / den
        ok = live[:, None] & torch.isfinite(den) & (den != 0) & (sg * nt >= 0) & (sg * nu >= 0) & (sg * nu <= sg * den) & (t <= MAX_RANGE)
        ok = ok & alive[:, self.origin].bool()[:, None, None]
        t = torch.where(ok, t, torch.full_like(t, float('inf')))
        best, at = t.min(dim=2)   # (equal distances: whichever edge min returns; the tool reports how many ids agree)
        hit = torch.isfinite(best)
        dist = torch.where(hit, best + 0.0, torch.full_like(best, MAX_RANGE))
        ids = torch.where(hit, self.row[at] + 1, torch.zeros_like(at))
        return torch.stack([dist, ids.double()], dim=2).float()


def wall(torch, call, steps):
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from moog import _abi, environment
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say('%d envs, %d timed calls each; %s' % (args.envs, args.steps, torch.cuda.get_device_name(0)))
    say('%-24s %5s %9s %10s %10s %10s %9s   %s' % ('workload', 'rays', 'ms/call', 'sensor us', 'step us', 'torch us', 'torch/us', 'agreement'))
    for name in WORKLOADS:
        for rays in RAYS:
            torch.manual_seed(0)
            env = environment.BatchedEnvironment(num_envs=args.envs, seed=1, **config(name, rays))
            env.check_faults = False
            env.reset()
            acts = [env.random_action() for _ in range(8)]
            k = [0]

            def step():
                k[0] += 1
                env.step(acts[k[0] % 8])
            ms = wall(torch, step, args.steps)
            env.set_timing(True, kernels=[_abi.MOOG_K_TABLES, _abi.MOOG_K_STEP])
            env.kernel_time(_abi.MOOG_K_TABLES)
            env.kernel_time(_abi.MOOG_K_STEP)
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            kms, n = env.kernel_time(_abi.MOOG_K_TABLES)
            sms, sn = env.kernel_time(_abi.MOOG_K_STEP)
            env.set_timing(False)
            us, sus = 1e3 * kms / max(1, n), 1e3 * sms / max(1, sn)
            ts = TorchSensor(env, torch)
            tus = 1e3 * wall(torch, ts, max(10, args.steps // 4))
            got, want = env.tables['rays'], ts()
            torch.cuda.synchronize()
            same_d = float((got[:, :, 0] == want[:, :, 0]).double().mean())
            same_i = float((got[:, :, 1] == want[:, :, 1]).double().mean())
            edges = int(ts.slot.numel())
            say('%-24s %5d %9.4f %10.1f %10.1f %10.1f %9.1f   distances equal %.6f, ids equal %.6f; %d edge slots per env'
                % (name, rays, ms, us, sus, tus, tus / us, same_d, same_i, edges))
            env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
