"""Builds the HIP engine in-tree: mate_amd/lib/libmate_engine.so (gfx950 only).

hipcc cross-compiles without a GPU.  -ffp-contract=off is part of the numerics
contract (see csrc/device_math.hpp); explicit fma() marks the fused products.
"""
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
SRC = os.path.join(CSRC, 'mate_engine.hip')
# The translation units in link order: (object, source under csrc/, extra defines, resource record under lib/).  mate_engine.hip (host
# side, generic kernels, reset) and one shape_group.hip per group of compiled scenario shapes (csrc/shape_groups.hpp) report into
# kernel_resources.json, which tests/test_kernel_resources.py pins name by name and figure by figure.  A kernel that arrives later leaves
# that record as it is: it comes in a unit of its own with a record of its own -- one row here, one entry in tests/test_unit_resources.py.
UNITS = [('mate_engine', 'mate_engine.hip', (), 'kernel_resources.json')]
UNITS += [(f'shape_group_{k}', 'shape_group.hip', (f'-DMATE_SHAPE_GROUP={k}',), 'kernel_resources.json') for k in range(6)]
UNITS += [('opponent_kernels', 'opponent_kernels.hip', (), 'kernel_resources_opponents.json'),      # heuristic_drift_kernel, heuristic_camera_kernel
          ('headline_kernels', 'headline_kernels.hip', (), 'kernel_resources_headline.json'),       # headline_rollout_kernel
          ('episode_kernels', 'episode_kernels.hip', (), 'kernel_resources_episodes.json'),         # episode_rows_kernel
          ('info_kernels', 'info_kernels.hip', (), 'kernel_resources_info.json'),                   # info_rows_kernel
          ('scripted_kernels', 'scripted_kernels.hip', (), 'kernel_resources_scripted.json'),       # scripted_opponent_kernel
          ('channel_kernels', 'channel_kernels.hip', (), 'kernel_resources_channel.json'),          # greedy_channel_kernel
          ('seat_kernels', 'seat_kernels.hip', (), 'kernel_resources_seat.json'),                   # greedy_seat_kernel, seat_rows_kernel
          ('message_kernels', 'message_kernels.hip', (), 'kernel_resources_message.json')]          # message_rows_kernel
# The units outside that table: compiled and linked with it, each with a record of its own that no test of the table's reads.  render_kernel came after
# tests/test_gpu_frame_fragments.py had pinned the set of kernels the opponents' record may gain, so it could join neither that unit nor the table.
LATER_UNITS = [('render_kernels', 'render_kernels.hip', (), 'render_resources.json')]                  # render_kernel
# ... and the units that came behind tests/test_render_host.py, which pins LATER_UNITS to its one row: a third list, compiled and linked with the others.
TRACE_UNITS = [('trace_kernels', 'trace_kernels.hip', (), 'trace_resources.json')]                    # comm_trace_kernel, trace_plant_kernel
# Everything the library is built from: the sources in csrc/ by suffix (no editor backup, no stray object) in sorted order -- the same
# digest on every machine -- and the public header.
DEPS = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if os.path.splitext(f)[1] in ('.hip', '.hpp', '.h', '.inc')) + [
    os.path.join(os.path.dirname(HERE), 'include', 'mate_engine.h')]
OUT = os.path.join(HERE, 'lib', 'libmate_engine.so')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared',
         # MachineLICM hoists every literal (polynomial coefficients, masks) out of the phase loops and pins
         # ~50 VGPRs for the whole kernel; without it step_kernel needs 52 VGPRs instead of 100
         '-mllvm', '-disable-machine-licm']


STAMP = os.path.join(HERE, 'lib', 'build_stamp.json')


def source_digest():
    """sha256 over the sources and the flags the library is built from."""
    import hashlib
    h = hashlib.sha256(' '.join(FLAGS).encode())
    for d in DEPS:
        with open(d, 'rb') as fh:
            h.update(os.path.basename(d).encode() + b'\0' + fh.read())
    return h.hexdigest()


def needs_build():
    """True unless the library in the tree was built from exactly these sources.  By CONTENT, not by modification time: a snapshot of
    the tree copied to another machine (gpurun, the driver's GPU tier) does not keep the order of the files' time stamps, and a
    time-based rule rebuilt the whole library there -- 40 s in front of every smoke() -- for nothing."""
    if not os.path.exists(OUT) or not os.path.exists(STAMP):
        return True
    try:
        with open(STAMP) as fh:
            return json.load(fh).get('sources') != source_digest()
    except (OSError, ValueError):
        return True


RESOURCES = os.path.join(HERE, 'lib', 'kernel_resources.json')      # (the engine's own record: UNITS)
_REMARK = re.compile(r'remark:\s+(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Dynamic Stack|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\S+)')


def parse_resources(text):
    """Per-kernel register / scratch / occupancy figures from the compiler's kernel-resource-usage remarks."""
    kernels, current = {}, None
    for key, value in _REMARK.findall(text):
        if key == 'Function Name':
            current = kernels.setdefault(value, {})
        elif current is not None:
            current[key.split(' [')[0]] = value if key == 'Dynamic Stack' else int(value)
    return kernels


def _compile_and_link(out, extra=(), verbose=False, remarks=False):
    """The engine's translation units (UNITS) compiled in parallel and linked into `out`.  Returns the compilers' stderr (remarks) per
    resource record, {record: text}, the units of one record concatenated in their order."""
    import concurrent.futures
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    objdir = os.path.join(os.path.dirname(OUT), 'obj', os.path.splitext(os.path.basename(out))[0])
    os.makedirs(objdir, exist_ok=True)
    compile_flags = [f for f in FLAGS if f != '-shared'] + list(extra) + (['-Rpass-analysis=kernel-resource-usage'] if remarks else [])
    units = UNITS + LATER_UNITS + TRACE_UNITS
    objects = [os.path.join(objdir, name + '.o') for name, _, _, _ in units]

    def compile_unit(unit, obj):
        cmd = [hipcc] + compile_flags + list(unit[2]) + ['-c', '-o', obj, os.path.join(CSRC, unit[1])]
        if verbose:
            print(' '.join(cmd), flush=True)
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        return cmd, done

    # (a fixed cap, not os.cpu_count(): a job on a shared machine may use far fewer CPUs than the machine reports)
    workers = max(1, int(os.environ.get('MATE_BUILD_JOBS', '0')) or min(len(units), 16))
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
        results = list(pool.map(compile_unit, units, objects))
    texts = {}
    for unit, (cmd, done) in zip(units, results):
        if done.returncode != 0:
            sys.stderr.write(done.stderr)
            raise subprocess.CalledProcessError(done.returncode, cmd)
        texts[unit[3]] = texts.get(unit[3], '') + done.stderr
    link = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', out] + objects
    if verbose:
        print(' '.join(link), flush=True)
    done = subprocess.run(link, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if done.returncode != 0:
        sys.stderr.write(done.stderr)
        raise subprocess.CalledProcessError(done.returncode, link)
    return texts


def build_engine(force=False, verbose=False):
    if not force and not needs_build():
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    bad = []
    for record, text in _compile_and_link(OUT, verbose=verbose, remarks=True).items():
        kernels = parse_resources(text)
        with open(os.path.join(HERE, 'lib', record), 'w') as f:
            json.dump(kernels, f, indent=1, sort_keys=True)
        # A kernel that needs private scratch memory (a spilled register, an outlined helper that takes the environment
        # context by reference) costs ~5 us more per LAUNCH than one that does not -- a third of the headline step.
        bad += [k for k, r in kernels.items() if r.get('ScratchSize', 0) != 0 or r.get('Dynamic Stack') != 'False']
    if bad:
        os.remove(OUT)
        raise RuntimeError('kernels with private scratch memory: ' + ', '.join(bad))
    with open(STAMP, 'w') as f:
        json.dump({'sources': source_digest()}, f)
    return OUT


def build_profiling(verbose=False):
    """The profiling build (per-wave s_memtime stamps at the phase boundaries, -DMATE_PHASE_CLOCKS): lib/libmate_engine_prof.so,
    selected with MATE_ENGINE_LIB by tools/*_phases.py.  Never loaded by the package itself."""
    out = os.path.join(HERE, 'lib', 'libmate_engine_prof.so')
    _compile_and_link(out, extra=['-DMATE_PHASE_CLOCKS'], verbose=verbose)
    return out


def build_tools(verbose=False):
    """The stand-alone measurement programs under tools/ (store rooflines, issue rates): one hipcc call each, binaries next to
    the sources (git-ignored; they travel to the GPU box with the tree)."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
    built = []
    for name in ('store_roof', 'store_bits', 'store_contig', 'store_vmm', 'region_bw', 'valu_rates', 'chunk_order', 'dispatch_probe', 'va_reuse', 'store_layout'):
        src, out = os.path.join(tools, name + '.hip'), os.path.join(tools, name)
        if not os.path.exists(src) or (os.path.exists(out) and os.path.getmtime(out) >= os.path.getmtime(src)):
            continue
        cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I' + os.path.dirname(SRC), '-o', out, src]
        if verbose:
            print(' '.join(cmd))
        subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        built.append(out)
    return built


def build_variant(name, defines, verbose=False):
    """An experiment build, lib/libmate_engine_<name>.so with extra -D flags (A/B partners of tools/rollout_ab.py and of
    MATE_ENGINE_LIB=...; never loaded by the package itself)."""
    out = os.path.join(HERE, 'lib', 'libmate_engine_%s.so' % name)
    _compile_and_link(out, extra=list(defines), verbose=verbose)
    return out


if __name__ == '__main__':
    if '--variant' in sys.argv:      # python -m mate_amd.build --variant NAME -DFLAG[=V] ...
        build_variant(sys.argv[sys.argv.index('--variant') + 1], [a for a in sys.argv if a.startswith('-D')], verbose=True)
        sys.exit(0)
    build_engine(force='--force' in sys.argv, verbose=True)
    if '--tools' in sys.argv:
        build_tools(verbose=True)
    if '--prof' in sys.argv:
        build_profiling(verbose=True)
