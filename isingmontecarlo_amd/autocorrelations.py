"""Autocorrelations of sampled observables (qmc::sse::autocorrelations, src/sse/autocorrelations.rs).

Post-processing of the p=0 states a batch samples.  The transform itself runs on the host (numpy FFT; the reference uses
rustfft) or, with `device="cuda"`, on the GPU through hipFFT (torch.fft on a ROCm build dispatches to hipFFT): the batched
form — every variable of every replica is one series — is what a 1024-replica batch needs.

Every observable the reference autocorrelates on an Ising graph is two-valued (a spin, a product of spins, a bond that is satisfied
or not), so with `device="record"` no transform runs at all: the sampled states stay on the GPU in the batch's sample record, the
series are bits, and the circular autocorrelation of a +-1 series is a population count (bit_autocorrelation below states the
arithmetic; csrc/sse_observe.hip.h runs it)."""
import numpy as np


def fft_autocorrelation_device(samples, device="cuda"):
    """The same as fft_autocorrelation for a whole batch at once on the GPU (hipFFT): `samples` is [T][R][n], returns [R][T].
    (A process that uses torch's HIP runtime next to this library must let torch touch the GPU first — `torch.cuda.is_available()`
    before the first batch is created, as bench.py does; the other order leaves torch without devices.)"""
    import torch
    x = torch.as_tensor(np.ascontiguousarray(samples), dtype=torch.float64, device=device)
    tmax, _, n = x.shape
    x = x - x.mean(dim=0, keepdim=True)
    norm = torch.sqrt((x * x).sum(dim=0, keepdim=True))
    x = torch.where(norm > 0, x / torch.where(norm > 0, norm, torch.ones_like(norm)), torch.zeros_like(x))
    f = torch.fft.fft(x, dim=0)
    ac = torch.fft.ifft(f * torch.conj(f), dim=0).real * tmax  # (rustfft's inverse is unnormalised)
    return (ac.sum(dim=2) / (n * tmax)).transpose(0, 1).contiguous().cpu().numpy()


def direct_autocorrelation(samples):
    """The defining circular sum, O(T^2) per observable: r[tau] = mean over observables of sum_t y[t] y[(t + tau) mod T] with y
    the centred, unit-norm series (test reference for the FFT forms)."""
    x = np.asarray(samples, dtype=np.float64)
    tmax, n = x.shape
    x = x - x.mean(axis=0, keepdims=True)
    norm = np.sqrt((x * x).sum(axis=0, keepdims=True))
    x = np.divide(x, norm, out=np.zeros_like(x), where=norm > 0)
    return np.array([(x * np.roll(x, -tau, axis=0)).sum() / n for tau in range(tmax)])


def fft_autocorrelation(samples):
    """fft_autocorrelation (autocorrelations.rs:99-133): `samples` is [T][n] (T samples of n observables).  Every
    observable is centred and scaled to unit norm, its circular autocorrelation is taken through the FFT, and the
    result is averaged over the n observables: returns T values, r[0] = 1 (up to rounding) when every observable varied."""
    x = np.asarray(samples, dtype=np.float64)
    tmax, n = x.shape
    x = x - x.mean(axis=0, keepdims=True)
    norm = np.sqrt((x * x).sum(axis=0, keepdims=True))
    x = np.divide(x, norm, out=np.zeros_like(x), where=norm > 0)  # an observable that never changed contributes 0 (the reference divides by 0 there)
    f = np.fft.fft(x, axis=0)
    ac = np.fft.ifft(f * np.conj(f), axis=0).real * tmax  # rustfft's inverse is unnormalised
    return ac.sum(axis=1) / (n * tmax)


def bit_autocorrelation(bits):
    """The autocorrelation of two-valued observables without transforms: `bits` is [T][n] of 0/1 (1 standing for +1), returns the
    same T values as fft_autocorrelation(2 * bits - 1).  For one observable x with s = sum_t x[t] = 2 ones - T and
    C(tau) = sum_t x[t] x[(t + tau) mod T] = T - 2 popcount(bits ^ rotate(bits, tau)), centring and unit norm
    (autocorrelations.rs:99-133) give (T C(tau) - s^2) / (T^2 - s^2): integers up to that one float64 division, 0 for an observable
    that never changed (T^2 == s^2).  The terms are added in observable order and the sum is divided by n once: the order
    of csrc/sse_observe.hip.h's bit_autocorr_kernel, whose result this restates bit for bit."""
    b = np.asarray(bits)
    if b.ndim != 2 or b.shape[0] == 0 or b.shape[1] == 0:
        raise ValueError("bits must be [T][n] with T, n >= 1")
    b = (b != 0)
    tmax, n = b.shape
    t = np.int64(tmax)
    s = 2 * b.sum(axis=0, dtype=np.int64) - t
    den = t * t - s * s
    live = den != 0
    fden = np.where(live, den, 1).astype(np.float64)
    acc = np.zeros(tmax, dtype=np.float64)
    num = np.empty((tmax, n), dtype=np.int64)
    for tau in range(tmax):
        ham = (b != np.roll(b, -tau, axis=0)).sum(axis=0, dtype=np.int64)
        num[tau] = t * (t - 2 * ham) - s * s
    for i in range(n):  # one division per term, terms added in observable order
        if live[i]:
            acc += num[:, i].astype(np.float64) / fden[i]
    return acc / np.float64(n)


def variable_groups(nvars):
    """Observable groups and flips (QmcIsingGraph.record_series) of the +-1 spins (autocorrelations.rs:37-50): {v}, no flip."""
    return [[v] for v in range(int(nvars))], np.zeros(int(nvars), dtype=np.uint8)


def product_groups(var_products):
    """... of products of +-1 spins (autocorrelations.rs:52-75): the product over vs is +1 iff the number of 0 bits is even, i.e.
    parity(bits) ^ (1 if len(vs) is even else 0)."""
    groups = [[int(v) for v in vs] for vs in var_products]
    return groups, np.array([1 - (len(g) & 1) for g in groups], dtype=np.uint8)


def bond_groups(graph):
    """... of the bonds (value_for_bond, qmc_ising.rs:988-997): bond e = (a, b) with coupling J is +1 iff the number of set bits
    among a, b is even for J < 0 and odd otherwise, i.e. parity ^ (1 if J < 0 else 0).  Bonds are the edges, in edge order (n_bonds,
    qmc_ising.rs:984-986).  A batch built by Qmc.from_interactions has matrix entries for bond values (qmc_runner.rs:746-750), not
    two values: ENOTIMPL."""
    if getattr(graph, "interactions", None) is not None:
        from . import IsingMcError
        raise IsingMcError(-5, "bond values of generic interactions are matrix entries, not two-valued (qmc_runner.rs:746-750)")
    j = np.asarray(graph.J, dtype=np.float64)
    if j.ndim != 1:
        from . import IsingMcError
        raise IsingMcError(-5, "bond observables need one coupling per edge (not per-replica couplings)")
    return [[int(a), int(b)] for a, b in np.asarray(graph.edges)], (j < 0).astype(np.uint8)


def bond_values(graph, states):
    """value_for_bond (qmc_ising.rs:988-997) for every bond: `states` is [...][N] of 0/1, returns float64 [...][n_bonds] of +-1."""
    groups, flips = bond_groups(graph)
    st = np.asarray(states).astype(np.uint8)
    e = np.asarray(groups, dtype=np.int64).reshape(-1, 2)
    bit = (st[..., e[:, 0]] ^ st[..., e[:, 1]] ^ flips) & 1
    return bit.astype(np.float64) * 2.0 - 1.0


def _sample_states(graph, timesteps, beta, sampling_freq):
    """The host path's sampling loop: one call and one state read-back per sample; returns uint8 [T][R][N]."""
    states = []
    done = 0
    while done < timesteps:
        t = min(sampling_freq, timesteps - done)
        graph.run(t, beta)
        done += t
        if done % sampling_freq == 0:
            states.append(graph.state_ref())
    return np.stack(states)


def _record_autocorrelation(graph, timesteps, beta, sampling_freq, groups, r):
    """device="record": the whole run in one call with the samples kept on the device, then the bit-series kernels.  Uses the
    attached record when it has room (the samples stay in it), else one of its own for the call."""
    nsamp = int(timesteps) // int(sampling_freq)
    have, cap = graph.record_count(), graph.record_capacity()
    own = cap - have < nsamp
    if own:
        if cap:
            from . import IsingMcError
            raise IsingMcError(-3, f"the attached sample record has room for {cap - have} of the {nsamp} samples")
        graph.attach_sample_record(max(nsamp, 1))
        have = 0
    try:
        graph.run(timesteps, beta, sampling_freq)
        out = graph.record_autocorrelation(groups, have, nsamp)
    finally:
        if own:
            graph.detach_sample_record()
    return out if r is None else out[r]


def bond_autocorrelation(graph, timesteps, beta, sampling_freq=1, r=None, device=None):
    """QmcBondAutoCorrelations::calculate_bond_autocorrelation (autocorrelations.rs:84-97): the observables are the bonds' values
    (+1 satisfied, -1 not).  device=None: host FFT per replica; "record": sample record and bit-series kernels; anything else:
    fft_autocorrelation_device on that device."""
    groups, _ = bond_groups(graph)
    if device == "record":
        return _record_autocorrelation(graph, timesteps, beta, sampling_freq, groups, r)
    vals = bond_values(graph, _sample_states(graph, timesteps, beta, sampling_freq))  # [T][R][n_bonds]
    if device is not None:
        out = fft_autocorrelation_device(vals if r is None else vals[:, r:r + 1, :], device)
        return out if r is None else out[0]
    reps = range(vals.shape[1]) if r is None else [r]
    out = np.stack([fft_autocorrelation(vals[:, k, :]) for k in reps])
    return out if r is None else out[0]


def variable_autocorrelation(graph, timesteps, beta, sampling_freq=1, r=None, device=None):
    """QmcAutoCorrelations::calculate_variable_autocorrelation (autocorrelations.rs:37-50) for a batch: runs `timesteps`
    sweeps, samples the p=0 states every `sampling_freq` sweeps and returns the autocorrelation of the +-1 spins, one
    row per replica (or for replica r only).  `device="cuda"`: the transforms of all replicas in one hipFFT batch;
    `device="record"`: one call for the whole run with the samples kept in the batch's sample record, then population counts."""
    if device == "record":
        return _record_autocorrelation(graph, timesteps, beta, sampling_freq, variable_groups(graph.nvars)[0], r)
    states = []
    done = 0
    while done < timesteps:
        t = min(sampling_freq, timesteps - done)
        graph.run(t, beta)
        done += t
        if done % sampling_freq == 0:
            states.append(graph.state_ref())
    st = np.stack(states).astype(np.float64) * 2.0 - 1.0  # [T][R][N]
    if device is not None:
        out = fft_autocorrelation_device(st if r is None else st[:, r:r + 1, :], device)
        return out if r is None else out[0]
    reps = range(st.shape[1]) if r is None else [r]
    out = np.stack([fft_autocorrelation(st[:, k, :]) for k in reps])
    return out if r is None else out[0]


def spin_product_autocorrelation(graph, timesteps, beta, var_products, sampling_freq=1, r=None, device=None):
    """calculate_spin_product_autocorrelation (autocorrelations.rs:52-75): observables are products of the +-1 spins of
    each variable group in `var_products`.  `device="record"`: as in variable_autocorrelation."""
    if device == "record":
        return _record_autocorrelation(graph, timesteps, beta, sampling_freq, product_groups(var_products)[0], r)
    states = []
    done = 0
    while done < timesteps:
        t = min(sampling_freq, timesteps - done)
        graph.run(t, beta)
        done += t
        if done % sampling_freq == 0:
            states.append(graph.state_ref())
    st = np.stack(states).astype(np.float64) * 2.0 - 1.0
    prods = np.stack([st[:, :, list(vs)].prod(axis=2) for vs in var_products], axis=2)  # [T][R][len(var_products)]
    if device is not None:
        out = fft_autocorrelation_device(prods if r is None else prods[:, r:r + 1, :], device)
        return out if r is None else out[0]
    reps = range(st.shape[1]) if r is None else [r]
    out = np.stack([fft_autocorrelation(prods[:, k, :]) for k in reps])
    return out if r is None else out[0]
