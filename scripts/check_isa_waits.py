"""Dev lint: compile the conv translation units to gfx950 assembly and flag any s_waitcnt vmcnt(...) the compiler
placed directly in front of a K-loop fragment-read cluster (>= 8 ds_read_b128) of an igemm_stagger_kernel or
igemm_wide_kernel.

Why: the staggered kernel keeps two K-tiles of LDS-DMA in flight with counted waits of its own.  Whether the compiler
adds a draining `s_waitcnt vmcnt(0)` before the fragment reads depends on its register scoreboard at the loop header
(a global load consumed only under a condition leaves "maybe pending" registers; re-using one of them inside the loop
forces the wait) -- it appeared and disappeared with unrelated edits during round 1.  Run after touching
igemm_stagger.hip.h / igemm_wide.hip.h / igemm.hip.h epilogues:   python scripts/check_isa_waits.py
Also checks the wgrad_patch.hip.h kernels (no scratch access between their MFMAs, accumulation in place), and the
persistent fc-GRU kernel (fcgru_seq.hip.h): in each of its two phases all 13 x NF sixteen-byte exchange loads of a wave
must stand in front of the phase's first MFMA (the scheduler, left alone, sinks them between the MFMAs and re-uses 2 - 4
registers: 2 - 3 loads in flight instead of the >= 8 the hand-off needs), and nothing may spill.  Sixteen instantiations
<NF, SAVE, STREAM>: the eight STREAM = false ones as before, and the eight streaming ones (step 0 of phase A on the seeded rows).
The persistent fc-GRU BPTT kernel (fcgru_bptt.hip.h), eight instantiations <NF, STREAM>, four of them streaming
(rgp_fcgru_backward_stream: n_valid steps from the seeded carry, the same step body): the same rule for each fcs_gemm call of the
step body -- GEMM C, the u half and the r half of GEMM ZR: three runs of exactly 13 x NF loads in front of 13 x NF MFMAs (no
phase of any instantiation issues its loads in two runs), and no scratch access.
The f32 persistent fc-GRU kernel (fcgru_seq_f32.hip.h), sixteen instantiations <NF, SAVE, STREAM>: a fragment's A operands are
26 sixteen-byte exchange loads and 104 MFMAs (v_mfma_f32_16x16x4_f32), and only two fragments' loads fit the register file, so
each phase issues its loads in GROUPS: fragments 0 and 1 (26 min(NF, 2) loads) in front of the first MFMA, then 26 loads of
fragment f + 2 behind the 104 MFMAs of fragment f.  Each group must stand in front of the MFMAs that consume it: the runs of a
phase are exactly [L 26 min(NF, 2), M 104] + [L 26, M 104] x (NF - 3) + [L 26, M 208] (NF <= 2: [L 26 NF, M 104 NF]), twice per
kernel, every exchange load 16 bytes wide, and no scratch access.
The f32 persistent fc-GRU BPTT kernel (fcgru_bptt_f32.hip.h), eight instantiations <NF, STREAM>, four of them streaming: a step
is three fcs32_gemm passes --
GEMM C (b_c from registers), the u half and the r half of GEMM ZR (both from LDS) -- so the runs of the f32 forward's phase are
expected exactly THREE times per kernel, every exchange load 16 bytes wide, and no scratch access.
"""
import os, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'recurrent_gaze_prediction_amd', 'csrc')


def kernels_named(asm, prefix, contains=''):
    """(symbol, body lines up to s_endpgm) of every kernel whose symbol starts with prefix (or one of a tuple) and contains `contains`."""
    lines = asm.split('\n')
    for st, l in enumerate(lines):
        if l.startswith(prefix) and contains in l and '@' in l:
            end = next(i for i in range(st, len(lines)) if 's_endpgm' in lines[i])
            yield l.split(':')[0], lines[st:end]


def stray_waits(body):
    i, bad = 0, []
    while i < len(body):
        if 'ds_read_b128' in body[i]:
            j = i
            while j < len(body) and ('ds_read_b128' in body[j] or 'v_add_u32' in body[j]):
                j += 1
            n = sum('ds_read_b128' in l for l in body[i:j])
            pre = [l.strip() for l in body[max(0, i - 14):i] if 'vmcnt' in l]
            if n >= 8 and pre:
                bad.append((i, pre))
            i = j
        else:
            i += 1
    return bad


def wgrad_patch_faults(body):
    """wgrad_patch.hip.h: between the first and the last MFMA there must be no scratch access (a spill inside the group
    loop waits on vmcnt and with it on the slab DMA in flight: +10 % when it happened), every MFMA must accumulate in
    place, and no compiler-inserted vmcnt wait may sit between two MFMAs of a step (the kernel's own are vmcnt(0) in
    front of a barrier)."""
    mf = [i for i, l in enumerate(body) if 'v_mfma' in l]
    faults = []
    if not mf:
        return ['no MFMA found']
    loop = body[mf[0]:mf[-1] + 1]
    if any('scratch_' in l for l in loop):
        faults.append('scratch access inside the MFMA region')
    for l in loop:
        if 'v_mfma' in l:
            ops = [o.strip() for o in l.split('v_mfma_f32_16x16x32_bf16')[1].split(',')]
            if ops[0] != ops[3]:
                faults.append('MFMA not in place: ' + l.strip())
                break
    return faults


def patch_faults(name, body):
    """conv_patch*.hip.h: no scratch access between the first and the last MFMA (a reload there waits on vmcnt and with it
    on the LDS-DMA ring), and -- inference kernels (no arg-max codes) -- none behind the last MFMA either: the round-3
    kernels lost 2-4 % to epilogue-only values the compiler had hoisted out of the tile loop and spilled across the K loop
    (each reload drained the look-ahead DMA once per tile)."""
    mf = [i for i, l in enumerate(body) if 'v_mfma' in l]
    sc = [i for i, l in enumerate(body) if 'scratch_load' in l]
    faults = []
    if any(mf[0] <= i <= mf[-1] for i in sc):
        faults.append('scratch reload inside the MFMA region')
    training = 'Lb1ELb1E' in name                      # <..., POOL = true, ARGMAX = true, ...>
    if not training and any(i > mf[-1] for i in sc):
        faults.append('scratch reload in the epilogue')
    return faults


def exchange_runs(body, mfma):
    """Runs of sc1 sixteen-byte exchange loads ('L') and of `mfma` instructions ('M') in program order -> (runs, faults); the
    faults are exchange loads narrower than 16 bytes and MFMAs of another kind."""
    runs, faults = [], []
    for l in body:
        k = 'L' if ('buffer_load_dwordx4' in l and 'sc1' in l) else 'M' if mfma in l else None
        if k is None and 'buffer_load' in l and 'sc1' in l:
            faults.append('exchange load narrower than 16 bytes: ' + l.strip())
        if k is None and 'v_mfma' in l:
            faults.append('an MFMA that is not %s: %s' % (mfma, l.strip()))
        if k and runs and runs[-1][0] == k:
            runs[-1][1] += 1
        elif k:
            runs.append([k, 1])
    return runs, faults


def bf16_phase(nf):
    """fcs_gemm: all 13 NF loads of a phase in front of its 13 NF MFMAs."""
    return [['L', 13 * nf], ['M', 13 * nf]]


def f32_phase(nf):
    """fcs32_gemm: the ring of two fragment buffers."""
    if nf <= 2:
        return [['L', 26 * nf], ['M', 104 * nf]]
    runs = [['L', 52], ['M', 104]]
    for f in range(1, nf - 1):                          # behind fragment f - 1: the loads of fragment f + 1
        runs += [['L', 26], ['M', 104 if f < nf - 2 else 208]]
    return runs


# (kernel, symbol prefix, instantiations, MFMA, runs of one phase, phases per kernel, what the summary line calls a fault, where
# the STREAM argument stands behind '_kernelILi', streaming instantiations expected)
BF16_WHAT = 'with exchange loads not in front of their MFMAs, or spills'
F32_WHAT = 'with a load group not in front of its MFMAs, narrow loads or spills'
FCGRU_RULES = [
    ('fcgru_seq', '_ZN3rgpL16fcgru_seq_kernel', 16, 'v_mfma_f32_16x16x32_bf16', bf16_phase, 2, BF16_WHAT, 5, 8),
    ('fcgru_bptt', '_ZN3rgpL17fcgru_bptt_kernel', 8, 'v_mfma_f32_16x16x32_bf16', bf16_phase, 3, BF16_WHAT, 1, 4),
    ('fcgru_seq_f32', '_ZN3rgpL20fcgru_seq_f32_kernel', 16, 'v_mfma_f32_16x16x4_f32', f32_phase, 2, F32_WHAT, 5, 8),
    ('fcgru_bptt_f32', '_ZN3rgpL21fcgru_bptt_f32_kernel', 8, 'v_mfma_f32_16x16x4_f32', f32_phase, 3, F32_WHAT, 1, 4),
]


def fcgru_faults(name, body, kernel, mfma, phase, n_phases):
    nf = int(name.split(kernel + '_kernelILi')[1][0])
    runs, faults = exchange_runs(body, mfma)
    if runs != phase(nf) * n_phases:
        faults.append('loads not in front of their MFMAs: ' + ' '.join('%s%d' % (k, n) for k, n in runs))
    if any('scratch_' in l for l in body):
        faults.append('scratch access')
    return faults[:3]


def compile_asm(tu):
    with tempfile.NamedTemporaryFile(suffix='.s') as tf:
        subprocess.run(['/opt/rocm/bin/hipcc', '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(ROOT, 'include'),
                        '-I' + CSRC, '-S', '--cuda-device-only', '-o', tf.name, os.path.join(CSRC, tu)], check=True,
                       stderr=subprocess.DEVNULL)
        return open(tf.name).read()


def main():
    rc = 0
    asm = compile_asm('rgp_fcgru.hip')
    for kernel, prefix, count, mfma, phase, n_phases, what, stream_at, count_stream in FCGRU_RULES:
        n = nbad = n_stream = 0
        for name, body in kernels_named(asm, prefix):
            n += 1
            # <NF, SAVE, STREAM>: the streaming instantiations (rgp_fcgru_forward_stream) run phase A of step 0 on the seeded rows
            # through the same GEMM call, so the same runs are expected of them; <NF, STREAM> (rgp_fcgru_backward_stream): the same
            # step body over n_valid steps
            n_stream += name.split('_kernelILi')[1][stream_at:].startswith('ELb1E')
            faults = fcgru_faults(name, body, kernel, mfma, phase, n_phases)
            if faults:
                nbad += 1
                print(kernel.upper(), name[:100], faults)
        print('rgp_fcgru.hip: %d %s kernels (%d streaming), %d %s' % (n, kernel, n_stream, nbad, what))
        rc |= nbad > 0 or n != count or n_stream != count_stream
    asm = compile_asm('rgp_conv_patch.hip')
    n = nbad = 0
    for name, body in kernels_named(asm, '_ZN3rgpL', 'conv_patch'):
        n += 1
        faults = patch_faults(name, body)
        if faults:
            nbad += 1
            print('CONV_PATCH', name[:100], faults)
    print('rgp_conv_patch.hip: %d patch kernels, %d with scratch reloads in the K loop / an inference epilogue' % (n, nbad))
    rc |= nbad > 0
    for tu in ('rgp_c3d.hip', 'rgp_c3d_bwd.hip'):
        asm = compile_asm(tu)
        n = nbad = 0
        for name, body in kernels_named(asm, ('_ZN3rgp20igemm_stagger_kernel', '_ZN3rgp17igemm_wide_kernel')):
            n += 1
            bad = stray_waits(body)
            if bad:
                nbad += 1
                print('STRAY WAIT', tu, name[:90], bad[:2])
        print('%s: %d staggered / wide kernels, %d with a compiler wait in front of the fragment reads' % (tu, n, nbad))
        rc |= nbad > 0
        nw = nwbad = 0
        for name, body in kernels_named(asm, '_ZN3rgpL23wgrad_patch_bf16_kernel'):
            nw += 1
            faults = wgrad_patch_faults(body)
            if faults:
                nwbad += 1
                print('WGRAD_PATCH', name[:90], faults)
        if nw:
            print('%s: %d wgrad_patch kernels, %d with spills in the loop or renamed accumulators' % (tu, nw, nwbad))
        rc |= nwbad > 0
    sys.exit(rc)


if __name__ == '__main__':
    main()
