"""What a Contacts observer costs (include/moog_engine.h moog_engine_add_contacts): colliding_predators_32 (32 x 32 pairs)
and falling_balls_64 (64 x 64) at 4096 envs, the config's own observers with and without one all-against-all
`Contacts(mode='pair')` --

  * the whole step() call without and with the observer, measured in the same run in alternating blocks (median of the
    blocks), and the HIP-event time of MOOG_K_TABLES per call with it (the contacts launch: the engine has no table or sensor);
  * the launch on its own (observe calls) over three states of the same records, so that R0 * R1 stays what it is while the
    candidate count moves: the records as stepped; every max_radius zeroed (the circle test rejects every pair: the fixed cost
    of the rows' prologue, the broad phase and the expansion to bytes); every sprite but the walls moved into one small disc
    (a crowd of candidates).  Candidates are counted here in torch with the kernel's broad phase (circle and 8-DOP with its
    margin; unordered pairs, as the kernel lists them when both arguments are the same list).

    python tools/bench_contacts.py [--envs 4096] [--steps 100] [--out profiles/contacts.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'moog.github.io_amd'))

WORKLOADS = ('colliding_predators_32', 'falling_balls_64')
MARGIN = 1e-5


def layers(name):
    from moog import _compiler
    from moog_demos import example_configs
    c = _compiler.compile_config(layer_capacity=example_configs.capacity(name), **example_configs.load(name))
    return tuple(k for k in c.layer_names if c.layer_slots[k][1] > 0)


def config(name, contacts):
    from moog import observers
    from moog_demos import example_configs
    cfg = example_configs.load(name)
    if contacts:
        cfg['observers'] = dict(cfg['observers'], touch=observers.Contacts(layers(name)))
    return cfg


class Records(object):
    """Views of an env's records for the candidate count and the planted states."""

    def __init__(self, env, torch):
        P, L = env.compiled.program, env.layout
        self.env, self.torch, self.L, self.S = env, torch, L, L.S
        dev = env.device
        cap = max(P.slot_vcap[s] for s in range(L.S))
        idx = [[P.slot_voff[s] + min(k, P.slot_vcap[s] - 1) for k in range(cap)] for s in range(L.S)]
        self.vidx = torch.tensor(idx, device=dev)                       # [S, cap] vertex numbers (clamped into the slot)
        self.k = torch.arange(cap, device=dev)[None, None, :]
        vslot = [0] * L.TOTV
        for s in range(L.S):
            for k in range(P.slot_vcap[s]):
                vslot[P.slot_voff[s] + k] = s
        self.vslot = torch.tensor(vslot, device=dev)                    # [TOTV] the slot of every vertex

    def parts(self):
        f, q, L, S = self.env.state_f64, self.env.state_i32, self.L, self.S
        alive = (q[:, L.o_flags:L.o_flags + S] & 1) != 0
        pos = f[:, L.o_pos:L.o_pos + 2 * S].view(-1, S, 2)
        maxr = f[:, L.o_maxr:L.o_maxr + S]
        verts = f[:, L.o_verts:L.o_verts + 2 * L.TOTV].view(-1, L.TOTV, 2)
        nv = q[:, L.o_nverts:L.o_nverts + S]
        return alive, pos, maxr, verts, nv

    def candidates(self):
        """[envs] unordered pairs of distinct live slots past the circle test and the 8-DOP test."""
        torch = self.torch
        alive, pos, maxr, verts, nv = self.parts()
        v = verts[:, self.vidx]                                         # [N, S, cap, 2]
        ok = self.k < nv[:, :, None]
        x, y = v[..., 0], v[..., 1]
        inf = float('inf')
        lo, hi = [], []
        for a in (x, y, x + y, x - y):
            lo.append(torch.where(ok, a, torch.full_like(a, inf)).amin(dim=2))
            hi.append(torch.where(ok, a, torch.full_like(a, -inf)).amax(dim=2))
        d = pos[:, :, None, :] - pos[:, None, :, :]
        near = ~(torch.sqrt(d[..., 1] * d[..., 1] + d[..., 0] * d[..., 0]) > maxr[:, :, None] + maxr[:, None, :])
        for l, h in zip(lo, hi):
            near &= ~(l[:, :, None] > h[:, None, :] + MARGIN) & ~(l[:, None, :] > h[:, :, None] + MARGIN)
        near &= alive[:, :, None] & alive[:, None, :]
        near &= torch.triu(torch.ones(self.S, self.S, dtype=torch.bool, device=near.device), diagonal=1)[None]
        return near.sum(dim=(1, 2))

    def cluster(self):
        """Every live sprite with max_radius below 0.2 (not the walls) moved, vertices and all, into a disc of radius 0.05."""
        torch = self.torch
        alive, pos, maxr, verts, nv = self.parts()
        g = torch.Generator(device='cpu').manual_seed(3)
        new = (0.5 + 0.1 * (torch.rand(pos.shape, generator=g, dtype=torch.float64) - 0.5)).to(pos.device)
        move = (alive & (maxr < 0.2))[:, :, None]
        d = torch.where(move, new - pos, torch.zeros_like(pos))
        verts += d[:, self.vslot]
        pos += d


def wall(torch, call, steps):
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
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from moog import _abi, environment
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say('%d envs, %d blocks of %d timed calls per engine, alternating; %s' % (args.envs, args.blocks, args.steps, torch.cuda.get_device_name(0)))
    for name in WORKLOADS:
        envs = {}
        for with_c in (False, True):
            torch.manual_seed(0)
            env = environment.BatchedEnvironment(num_envs=args.envs, seed=1, **config(name, with_c))
            env.check_faults = False
            env.reset()
            envs[with_c] = env
        acts = [envs[False].random_action() for _ in range(8)]
        k = [0]

        def stepper(env):
            def step():
                k[0] += 1
                env.step(acts[k[0] % 8])
            return step
        steps = {w: stepper(e) for w, e in envs.items()}
        for w in (False, True):
            wall(torch, steps[w], 20)   # warm-up
        ms = {False: [], True: []}
        for _ in range(args.blocks):
            for w in (False, True):
                ms[w].append(wall(torch, steps[w], args.steps))
        env = envs[True]
        shape = tuple(env.tables['touch'].shape[1:])
        env.set_timing(True, kernels=[_abi.MOOG_K_TABLES, _abi.MOOG_K_STEP])
        env.kernel_time(_abi.MOOG_K_TABLES)
        env.kernel_time(_abi.MOOG_K_STEP)
        for _ in range(args.steps):
            steps[True]()
        torch.cuda.synchronize()
        kms, n = env.kernel_time(_abi.MOOG_K_TABLES)
        sms, sn = env.kernel_time(_abi.MOOG_K_STEP)
        m0, m1 = statistics.median(ms[False]), statistics.median(ms[True])
        say('')
        say('%s, Contacts %d x %d (%d bytes an env)' % (name, shape[0], shape[1], shape[0] * shape[1]))
        say('  step() call   without %.4f ms (blocks %s)' % (m0, ' '.join('%.4f' % v for v in ms[False])))
        say('                with    %.4f ms (blocks %s)' % (m1, ' '.join('%.4f' % v for v in ms[True])))
        say('                added   %+.4f ms = %+.1f %% of the observer-free call' % (m1 - m0, 100.0 * (m1 - m0) / m0))
        say('  HIP events    MOOG_K_TABLES %.1f us per call over %d calls; MOOG_K_STEP %.1f us per call'
            % (1e3 * kms / max(1, n), n, 1e3 * sms / max(1, sn)))
        rec = Records(env, torch)
        say('  the launch on its own (MOOG_K_TABLES per observe call), R0 * R1 = %d throughout:' % (shape[0] * shape[1]))
        say('    %-34s %12s %12s %12s %14s' % ('state of the records', 'cand mean', 'cand max', 'us / call', 'flags set mean'))
        L, S = env.layout, env.layout.S
        rows = []
        for state in ('as stepped', 'max_radius zeroed: no candidate', 'clustered'):
            if state.startswith('max_radius'):
                keep = env.state_f64[:, L.o_maxr:L.o_maxr + S].clone()
                env.state_f64[:, L.o_maxr:L.o_maxr + S] = 0.0
            elif state == 'clustered':
                env.state_f64[:, L.o_maxr:L.o_maxr + S] = keep
                rec.cluster()
            cand = rec.candidates().double()
            env.kernel_time(_abi.MOOG_K_TABLES)
            for _ in range(args.steps):
                env._observe_tables()
            torch.cuda.synchronize()
            oms, on = env.kernel_time(_abi.MOOG_K_TABLES)
            us = 1e3 * oms / max(1, on)
            rows.append((float(cand.mean()), us))
            say('    %-34s %12.1f %12d %12.1f %14.1f' % (state, float(cand.mean()), int(cand.max()), us,
                                                          float(env.tables['touch'].sum()) / args.envs))
        fixed = rows[1][1]
        for (c, us), label in ((rows[0], 'as stepped'), (rows[2], 'clustered')):
            if c > 0:
                say('    %-12s (us - us of no candidate) / mean candidates = %.3f us per candidate and env-batch'
                    % (label, (us - fixed) / c))
        env.set_timing(False)
        for e in envs.values():
            e.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
