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
SRC = os.path.join(HERE, 'csrc', 'mate_engine.hip')
DEPS = [SRC] + [os.path.join(HERE, 'csrc', f) for f in ('engine_kernels.hpp', 'reset_kernels.hpp', 'policy_kernels.hpp', 'aux_kernels.hpp', 'attached_tile.hpp', 'state_rows.hpp', 'reward_rows.hpp', 'fragment_rows.hpp', 'selection_rows.hpp', 'device_math.hpp', 'instrument.hpp',
                                                          'shape_groups.hpp', 'shape_group.inc', 'shape_group.hip', 'engine_host.h', 'opponent_host.inc',
                                                          'opponent_rows.hpp', 'opponent_kernels.inc', 'opponent_kernels.hip',
                                                          'headline_kernels.hpp', 'headline_kernels.hip',
                                                          'episode_rows.hpp', 'episode_kernels.hip',
                                                          'info_rows.hpp', 'info_kernels.hip',
                                                          'scripted_rows.hpp', 'scripted_kernels.hip',
                                                          'channel_rows.hpp', 'channel_kernels.hip',
                                                          'seat_rows.hpp', 'seat_kernels.hip',
                                                          'message_rows.hpp', 'message_kernels.hip', 'message_host.inc')] + [
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


RESOURCES = os.path.join(HERE, 'lib', 'kernel_resources.json')
# The opponents' unit (csrc/opponent_kernels.hip) reports apart: kernel_resources.json is pinned, name by name and figure by figure, by
# tests/test_kernel_resources.py; kernels that arrive in a unit of their own leave that record as it is and are checked by their own test.
OPPONENT_SRC = os.path.join(HERE, 'csrc', 'opponent_kernels.hip')
OPPONENT_RESOURCES = os.path.join(HERE, 'lib', 'kernel_resources_opponents.json')
# ... and so does the headline's unit (csrc/headline_kernels.hip: headline_rollout_kernel, tests/test_headline_resources.py)
HEADLINE_SRC = os.path.join(HERE, 'csrc', 'headline_kernels.hip')
HEADLINE_RESOURCES = os.path.join(HERE, 'lib', 'kernel_resources_headline.json')
# ... and the episode records' (csrc/episode_kernels.hip: episode_rows_kernel, tests/test_episode_host.py)
EPISODE_SRC = os.path.join(HERE, 'csrc', 'episode_kernels.hip')
EPISODE_RESOURCES = os.path.join(HERE, 'lib', 'kernel_resources_episodes.json')
# ... and the training-information rows' (csrc/info_kernels.hip: info_rows_kernel, tests/test_info_rows_host.py)
INFO_SRC = os.path.join(HERE, 'csrc', 'info_kernels.hip')
INFO_RESOURCES = os.path.join(HERE, 'lib', 'kernel_resources_info.json')
# ... and the scripted opponents' and mixtures' (csrc/scripted_kernels.hip: scripted_opponent_kernel, tests/test_scripted_host.py)
SCRIPTED_SRC = os.path.join(HERE, 'csrc', 'scripted_kernels.hip')
SCRIPTED_RESOURCES = os.path.join(HERE, 'lib', 'kernel_resources_scripted.json')
# ... and the communication channels' (csrc/channel_kernels.hip: greedy_channel_kernel, tests/test_channel_host.py)
CHANNEL_SRC = os.path.join(HERE, 'csrc', 'channel_kernels.hip')
CHANNEL_RESOURCES = os.path.join(HERE, 'lib', 'kernel_resources_channel.json')
# ... and the learner seat's (csrc/seat_kernels.hip: greedy_seat_kernel, seat_rows_kernel, tests/test_seat_host.py)
SEAT_SRC = os.path.join(HERE, 'csrc', 'seat_kernels.hip')
SEAT_RESOURCES = os.path.join(HERE, 'lib', 'kernel_resources_seat.json')
# ... and the learner's messages' (csrc/message_kernels.hip: message_rows_kernel, tests/test_message_host.py)
MESSAGE_SRC = os.path.join(HERE, 'csrc', 'message_kernels.hip')
MESSAGE_RESOURCES = os.path.join(HERE, 'lib', 'kernel_resources_message.json')
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


N_SHAPE_GROUPS = 6      # csrc/shape_groups.hpp: the compiled scenario shapes in six groups, one translation unit each


def _compile_and_link(out, extra=(), verbose=False, remarks=False):
    """The engine as fifteen translation units compiled in parallel -- mate_engine.hip (host side, generic kernels, reset), one
    shape_group.hip per group of compiled scenario shapes, opponent_kernels.hip, headline_kernels.hip, episode_kernels.hip,
    info_kernels.hip, scripted_kernels.hip, channel_kernels.hip, seat_kernels.hip and message_kernels.hip -- and linked into `out`.  Returns the compilers'
    stderr (remarks) as a nonuple: of the engine's units, of the opponents' unit, of the headline's unit, of the episode records' unit, of the
    training-information rows' unit, of the scripted opponents' unit, of the communication channels' unit, of the learner seat's unit, of the
    learner's messages' unit."""
    import concurrent.futures
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    objdir = os.path.join(os.path.dirname(OUT), 'obj', os.path.splitext(os.path.basename(out))[0])
    os.makedirs(objdir, exist_ok=True)
    compile_flags = [f for f in FLAGS if f != '-shared'] + list(extra) + ['-DMATE_SPLIT_BUILD'] + (['-Rpass-analysis=kernel-resource-usage'] if remarks else [])
    units = [(SRC, [], os.path.join(objdir, 'mate_engine.o'))]
    units += [(os.path.join(HERE, 'csrc', 'shape_group.hip'), [f'-DMATE_SHAPE_GROUP={k}'], os.path.join(objdir, f'shape_group_{k}.o')) for k in range(N_SHAPE_GROUPS)]
    units += [(OPPONENT_SRC, [], os.path.join(objdir, 'opponent_kernels.o'))]
    units += [(HEADLINE_SRC, [], os.path.join(objdir, 'headline_kernels.o'))]
    units += [(EPISODE_SRC, [], os.path.join(objdir, 'episode_kernels.o'))]
    units += [(INFO_SRC, [], os.path.join(objdir, 'info_kernels.o'))]
    units += [(SCRIPTED_SRC, [], os.path.join(objdir, 'scripted_kernels.o'))]
    units += [(CHANNEL_SRC, [], os.path.join(objdir, 'channel_kernels.o'))]
    units += [(SEAT_SRC, [], os.path.join(objdir, 'seat_kernels.o'))]
    units += [(MESSAGE_SRC, [], os.path.join(objdir, 'message_kernels.o'))]

    def compile_unit(unit):
        src, defs, obj = unit
        cmd = [hipcc] + compile_flags + defs + ['-c', '-o', obj, src]
        if verbose:
            print(' '.join(cmd), flush=True)
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        return cmd, done

    workers = max(1, min(len(units), int(os.environ.get('MATE_BUILD_JOBS', '0')) or (os.cpu_count() or 2)))
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
        results = list(pool.map(compile_unit, units))
    text, opponent_text, headline_text, episode_text, info_text, scripted_text, channel_text, seat_text, message_text = '', '', '', '', '', '', '', '', ''
    for (src, _, _), (cmd, done) in zip(units, results):
        if done.returncode != 0:
            sys.stderr.write(done.stderr)
            raise subprocess.CalledProcessError(done.returncode, cmd)
        if src == OPPONENT_SRC:
            opponent_text += done.stderr
        elif src == HEADLINE_SRC:
            headline_text += done.stderr
        elif src == EPISODE_SRC:
            episode_text += done.stderr
        elif src == INFO_SRC:
            info_text += done.stderr
        elif src == SCRIPTED_SRC:
            scripted_text += done.stderr
        elif src == CHANNEL_SRC:
            channel_text += done.stderr
        elif src == SEAT_SRC:
            seat_text += done.stderr
        elif src == MESSAGE_SRC:
            message_text += done.stderr
        else:
            text += done.stderr
    link = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', out] + [u[2] for u in units]
    if verbose:
        print(' '.join(link), flush=True)
    done = subprocess.run(link, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if done.returncode != 0:
        sys.stderr.write(done.stderr)
        raise subprocess.CalledProcessError(done.returncode, link)
    return text, opponent_text, headline_text, episode_text, info_text, scripted_text, channel_text, seat_text, message_text


def build_engine(force=False, verbose=False):
    if not force and not needs_build():
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    text, opponent_text, headline_text, episode_text, info_text, scripted_text, channel_text, seat_text, message_text = _compile_and_link(OUT, verbose=verbose, remarks=True)
    kernels, opponents, headline, episodes = parse_resources(text), parse_resources(opponent_text), parse_resources(headline_text), parse_resources(episode_text)
    info, scripted, channel, seat = parse_resources(info_text), parse_resources(scripted_text), parse_resources(channel_text), parse_resources(seat_text)
    message = parse_resources(message_text)
    for path, table in ((RESOURCES, kernels), (OPPONENT_RESOURCES, opponents), (HEADLINE_RESOURCES, headline), (EPISODE_RESOURCES, episodes), (INFO_RESOURCES, info), (SCRIPTED_RESOURCES, scripted), (CHANNEL_RESOURCES, channel), (SEAT_RESOURCES, seat), (MESSAGE_RESOURCES, message)):
        with open(path, 'w') as f:
            json.dump(table, f, indent=1, sort_keys=True)
    # A kernel that needs private scratch memory (a spilled register, an outlined helper that takes the environment
    # context by reference) costs ~5 us more per LAUNCH than one that does not -- a third of the headline step.
    bad = [k for k, r in list(kernels.items()) + list(opponents.items()) + list(headline.items()) + list(episodes.items()) + list(info.items()) + list(scripted.items()) + list(channel.items()) + list(seat.items()) + list(message.items()) if r.get('ScratchSize', 0) != 0 or r.get('Dynamic Stack') != 'False']
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
