"""A many-lane host model of the reverse-mode programs of aehmc_amd/tracing.py (`_RevGen`): the emitted
``aehmc_logp_grad`` compiled as a stand-alone C++20 program and run by one ``std::thread`` per lane, 64 lanes (a
wavefront per chain) or 512 (a workgroup per chain), on one shared position row ``q`` and one shared, zeroed gradient
row ``g`` -- the way the engine's kernels run it.  The four macros the generated prelude leaves open are defined here:

  AEHMC_LANES             a variable (argv[1]): one build serves every lane count -- and 1, the loops run whole by one
                          thread, which is the one-lane program the many-lane results are compared with
  AEHMC_WSUM(x)           an all-reduce over a std::barrier: every lane deposits x, and behind the barrier forms the sum in
                          the device's order -- the xor butterfly m = 32 ... 1 within each 64-lane wavefront, then the
                          wavefronts' sums added in wavefront order (aehmc_wsum_ in _REV_PRELUDE); a second barrier before
                          the slots are used again
  AEHMC_SYNC()            a barrier, at EVERY lane count
  AEHMC_ATOMIC_ADD(p, v)  std::atomic_ref<double>(*p).fetch_add(v, relaxed)

What this models is the EIGHT-wavefront case: between two AEHMC_SYNC()s the lanes run in any order.  On the device one
wavefront runs in lock step and its LDS operations issue in order, so some interleavings the threads here can take do
not exist there; nothing of that is modelled, and a program that is clean here is clean on one wavefront a fortiori.
(AEHMC_SYNC() is empty on one wavefront on the device and a barrier here, for the same reason.)

The program prints the log-density and g, 17 digits each, and fails (exit status 3) if the lanes do not all return the
same bits.  It runs under a time limit: a WSUM or SYNC that only some lanes reach would hang the barrier, and a
timeout is a failure.  Built with -fsanitize=thread, every unordered pair of a write and another lane's access to one
entry is a ThreadSanitizer report -- which a comparison of values sees once in many runs, if ever.  The sanitizer runs
on this host program alone: nothing is preloaded, nothing runs through Python or on a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME_LIMIT = 60.0  # seconds, per run

# the part every model shares -- threads, barrier, reductions, atomics, main -- is one object file per set of flags
# (the standard headers are most of a build's time); a model's own file includes <cmath> and dual.cuh alone
HARNESS = r"""
#include <atomic>
#include <barrier>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
extern const int model_dim;
extern const double model_q[];
extern double model_g[];
double model_logp_grad(const double *q, double *g, int lane);
namespace simt {
int lanes = 64;
static std::barrier<> *bar;
static double *slot;
static thread_local int lane;
void sync() { bar->arrive_and_wait(); }
void atomic_add(double *p, double v) { std::atomic_ref<double>(*p).fetch_add(v, std::memory_order_relaxed); }
double wsum(double x) {
  if (lanes == 1) return x;  // (one lane: the loops run whole, the reductions are identities)
  slot[lane] = x;
  sync();
  double total = 0.0, mine = 0.0;
  for (int w = 0; w < lanes / 64; w++) {  // every wavefront's butterfly, by every lane: no lane waits for another's result
    double v[64], t[64];
    for (int l = 0; l < 64; l++) v[l] = slot[64 * w + l];
    for (int m = 32; m >= 1; m >>= 1) {
      for (int l = 0; l < 64; l++) t[l] = v[l] + v[l ^ m];
      std::memcpy(v, t, sizeof v);
    }
    if (w == lane / 64) mine = v[lane & 63];
    total = w == 0 ? v[0] : total + v[0];  // (aehmc_part[w]: what lane 0 of wavefront w holds)
  }
  sync();
  return lanes == 64 ? mine : total;
}
}
int main(int argc, char **argv) {
  const int D = model_dim;
  const int L = simt::lanes = argc > 1 ? std::atoi(argv[1]) : 64;
  if (L != 1 && (L < 64 || L % 64)) { std::fprintf(stderr, "lanes: 1 or a multiple of 64\n"); return 2; }
  std::barrier<> bar(L);
  std::vector<double> slot(L), ret(L);
  simt::bar = &bar;
  simt::slot = slot.data();
  std::vector<std::thread> th;
  for (int l = 0; l < L; l++)
    th.emplace_back([l, &ret] { simt::lane = l; ret[l] = model_logp_grad(model_q, model_g, l); });
  for (auto &t : th) t.join();
  for (int l = 1; l < L; l++)
    if (std::memcmp(&ret[l], &ret[0], sizeof(double))) {
      std::fprintf(stderr, "lane %d returns %.17g, lane 0 %.17g\n", l, ret[l], ret[0]);
      return 3;
    }
  std::printf("%.17g\n", ret[0]);
  for (int i = 0; i < D; i++) std::printf("%.17g\n", model_g[i]);
  return 0;
}
"""

MODEL = r"""
#include <cmath>
#define __device__
namespace simt {
extern int lanes;
void sync();
double wsum(double x);
void atomic_add(double *p, double v);
}
#define AEHMC_LANES simt::lanes
#define AEHMC_WSUM(x) simt::wsum(x)
#define AEHMC_SYNC() simt::sync()
#define AEHMC_ATOMIC_ADD(p, v) simt::atomic_add((p), (v))
#include "dual.cuh"
%(source)s
%(params)s
extern const int model_dim = %(D)d;
extern const double model_q[] = {%(q)s};
double model_g[%(D)d];
double model_logp_grad(const double *q, double *g, int lane) { return aehmc_logp_grad(q, g, lane, prm); }
"""

RACE_PROBE = r"""
#include <thread>
int x;
int main() { std::thread a([] { x = 1; }), b([] { x = 2; }); a.join(); b.join(); return 0; }
"""


def params_decl(tr):
    params = "".join(f"static const double prm{k}[] = {{{', '.join(repr(float(x)) for x in p)}}};\n" for k, p in enumerate(tr.params))
    return params + "static const double *const prm[] = {" + ", ".join([f"prm{k}" for k in range(len(tr.params))] + ["nullptr"]) + "};\n"


def _flags(tsan):
    # (-g1: line numbers in the sanitizer's reports, which name the two statements of a race)
    return ["-std=c++20", "-O1", "-pthread", *(["-fsanitize=thread", "-g1"] if tsan else []), "-I", os.path.join(ROOT, "aehmc_amd", "csrc")]


def _side_by_side(commands):
    procs = [(cmd, subprocess.Popen(cmd)) for cmd in commands]
    for cmd, p in procs:
        if p.wait():
            raise subprocess.CalledProcessError(p.returncode, cmd)


def harness_objects(directory, tsan):
    """the shared part, compiled once per directory and set of flags (one per entry of `tsan`)"""
    src = os.path.join(str(directory), "simt_harness.cpp")
    if not os.path.exists(src):
        with open(src, "w") as f:
            f.write(HARNESS)
    objs = [os.path.join(str(directory), "simt_harness_tsan.o" if t else "simt_harness.o") for t in tsan]
    _side_by_side([["g++", *_flags(t), "-c", "-o", obj, src] for t, obj in zip(tsan, objs) if not os.path.exists(obj)])
    return objs


def build(tr, q, directory, name, tsan=(False,)):
    """compile the reverse-mode program of the traced density `tr` at the position `q`, once per entry of `tsan` (False:
    the plain build, True: -fsanitize=thread), side by side; returns the executables' paths in that order"""
    src = os.path.join(str(directory), f"{name}_lanes.cpp")
    with open(src, "w") as f:
        f.write(MODEL % dict(source=tr.grad_source, params=params_decl(tr), D=len(q), q=", ".join(repr(float(x)) for x in q)))
    exes = [os.path.join(str(directory), f"{name}_lanes" + ("_tsan" if t else "")) for t in tsan]
    _side_by_side([["g++", *_flags(t), "-o", exe, src, obj] for t, exe, obj in zip(tsan, exes, harness_objects(directory, tsan))])
    return exes


def run(jobs):
    """jobs = [(executable, lanes)], started together -> [(exit status, stdout, stderr)]; a run over the time limit is an
    AssertionError"""
    procs = [subprocess.Popen([exe, str(lanes)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for exe, lanes in jobs]
    out = []
    try:
        for (exe, lanes), p in zip(jobs, procs):
            try:
                o, e = p.communicate(timeout=TIME_LIMIT)
            except subprocess.TimeoutExpired:
                raise AssertionError(f"{exe} on {lanes} lanes: no end within {TIME_LIMIT:.0f} s (a reduction or a barrier that only some lanes reach?)")
            out.append((p.returncode, o, e))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    return out


def value_and_gradient(result):
    """of one entry of run()'s; anything but exit status 0 is an AssertionError"""
    import numpy as np
    code, out, err = result
    assert code == 0, (code, err[-2000:])
    x = [float(s) for s in out.split()]
    return x[0], np.array(x[1:])


def tsan_probe(directory):
    """None if -fsanitize=thread works on this host -- a deliberate race between two threads compiles, links, starts and
    is reported -- else the reason it does not"""
    src = os.path.join(str(directory), "race_probe.cpp")
    with open(src, "w") as f:
        f.write(RACE_PROBE)
    exe = os.path.join(str(directory), "race_probe")
    c = subprocess.run(["g++", "-std=c++20", "-O1", "-pthread", "-fsanitize=thread", "-g", "-o", exe, src], capture_output=True, text=True)
    if c.returncode:
        return "g++ -fsanitize=thread does not build here: " + c.stderr.strip()[-300:]
    try:
        p = subprocess.run([exe], capture_output=True, text=True, timeout=TIME_LIMIT)
    except subprocess.TimeoutExpired:
        return "a ThreadSanitizer program does not finish on this host"
    if "WARNING: ThreadSanitizer: data race" not in p.stderr or p.returncode == 0:
        return f"ThreadSanitizer does not start or does not report a deliberate race on this host (exit status {p.returncode}): " + p.stderr.strip()[-300:]
    return None
