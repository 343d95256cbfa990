"""What the two device mixture fits share (codes/vbgmm.py: variational Bayes on t, codes/emgmm.py: EM on z): the single-process
communicator, the k-means labels of a cold start (on the gathered samples of rank 0: sklearn.cluster.KMeans on the host, exactly the call
BaseMixture._initialize_parameters makes, or with kmeans_backend="hip" / "hip_wide" the same algorithm on the device, codes/kmeans.py), fit_sliced -- the one
driver of the EM, the narrow sharded and the wide variational fit -- with the loop that drives its E-step / all-reduce / M-step launches against
the device-side `done` flag, the choice among `n_init` restarts and sklearn's messages.
"""
import collections
import warnings

import numpy as np
import torch

from .. import mixture_forms as FORMS

ILL_DEFINED = ("Fitting the mixture model failed because some components have ill-defined empirical covariance "
               "(for instance caused by singleton or collapsed samples). Try to decrease the number of "
               "components, increase reg_covar, or scale the input data.")
NOT_CONVERGED = ("Best performing initialization did not converge. Try different init parameters, or increase max_iter, "
                 "tol, or check for degenerate data.")


# Both state vectors end with the same four doubles (csrc/fit_util.h): lower_bound_, n_iter_, converged_ (-1 = ill-defined covariance), done;
# as indices from the end, so that state[FIT_CONVERGED:] = converged_ and done, state[FIT_DONE:] = the one-element view of the flag
FIT_LB, FIT_NITER, FIT_CONVERGED, FIT_DONE = -4, -3, -2, -1


class OneRank:
    """The communicator of a single-process fit: every exchange is the identity."""
    on, rank, world = False, 0, 1

    @staticmethod
    def allreduce_(t):
        return t

    @staticmethod
    def broadcast_(t, src):
        return t


def device_samples(X, device):
    """[N, R] fp32, contiguous, on `device`, from a torch tensor (preferred) or anything array-like."""
    Xd = X if isinstance(X, torch.Tensor) else torch.as_tensor(np.asarray(X, dtype=np.float32))
    return Xd.to(device=device, dtype=torch.float32).contiguous()


def check_sample_count(n, K):
    if n < K:
        raise ValueError("Expected n_samples >= n_components but got n_components = %d, n_samples = %d" % (K, n))


def kmeans_labels(X_host, K, rs):
    from sklearn import cluster
    return cluster.KMeans(n_clusters=K, n_init=1, random_state=rs).fit(X_host).labels_.astype(np.int32)


def kmeans_draws(rs, N, K):
    """The random numbers of ONE k-means++ seeding, taken from `rs` exactly as sklearn's _kmeans_plusplus takes them (tests/test_kmeans_cpu.py
    compares the generator's state with the one a sklearn fit leaves behind): the index of the first centre from rs.choice with uniform weights,
    then per further centre one rs.uniform(size=n_trials), n_trials = 2 + int(ln K).  -> (first index, uniforms [K-1, n_trials])."""
    n_trials = 2 + int(np.log(K))
    first = int(rs.choice(N, p=np.ones(N) / N))
    u = np.empty((K - 1, n_trials))
    for c in range(K - 1):
        u[c] = rs.uniform(size=n_trials)
    return first, u


def device_kmeans_labels(X_dev, K, rs):
    """kmeans_labels on the device: X_dev [N,R] stays where it is, -> int32 device tensor [N] (csrc/kmeans.hip)."""
    from .kmeans import DeviceKMeans
    return DeviceKMeans(n_clusters=K, n_init=1, random_state=rs, device=X_dev.device).fit(X_dev).labels_dev


KMEANS_BACKENDS = ("sklearn", "hip", "hip_wide")     # both device words mean DeviceKMeans, which picks its kernel family by the samples' width
DEVICE_KMEANS_BACKENDS = ("hip", "hip_wide")


def check_kmeans_backend(backend):
    if backend not in KMEANS_BACKENDS:
        raise ValueError("kmeans_backend must be one of %r, got %r" % (KMEANS_BACKENDS, backend))
    return backend


GM_FIT_DEVICE_BACKENDS = ("hip", "hip_wide")     # "hip": the narrow kernels alone; "hip_wide" (prior "GMM"): whichever family takes the width


def check_device_fit_width(config):
    """prior "GMM" fits its mixture on z, so the mixture dimension is code_size.  gm_fit_backend "hip" and kmeans_backend "hip" end at 64 dimensions
    (beyond: the host fits, which are the defaults, or "hip_wide"); "hip_wide" is the device EM fit, and as kmeans_backend the device k-means, of prior
    "GMM" at every width a kernel family takes (mixture_forms.EM_WIDTH_RULE).  For the other priors kmeans_backend "hip_wide" means "hip".  Raises
    ValueError naming the config key that asks for what does not exist.  (prior "ours": codes/vbgmm.py checks its own width.)"""
    fits = lambda: FORMS.EM_NARROW.takes(int(config["code_size"])) or FORMS.EM_WIDE.takes(int(config["code_size"]))     # (the device k-means: the same widths)
    if config.get("kmeans_backend") == "hip_wide" and config.get("prior") == "GMM" and not fits():
        raise ValueError('kmeans_backend: "hip_wide" clusters samples of %s, prior "GMM" with code_size = %d needs the host k-means '
                         '(leave kmeans_backend out or set it to "sklearn")' % (FORMS.EM_WIDTH_RULE, int(config["code_size"])))
    if config.get("gm_fit_backend") == "hip_wide":
        if config.get("prior") != "GMM":
            raise ValueError('gm_fit_backend: "hip_wide" is the device EM fit of prior "GMM", not of prior %r (use "hip" or "sklearn" there)'
                             % (config.get("prior"),))
        if not fits():
            raise ValueError('gm_fit_backend: "hip_wide" fits mixtures on %s, prior "GMM" with code_size = %d needs the host fit '
                             '(leave gm_fit_backend out or set it to "sklearn")' % (FORMS.EM_WIDTH_RULE, int(config["code_size"])))
    if config.get("prior") != "GMM" or int(config["code_size"]) <= FORMS.EM_NARROW.hi:
        return
    for key in ("gm_fit_backend", "kmeans_backend"):
        if config.get(key) == "hip":
            hint = ' or, for a device %s on %d .. %d dimensions in steps of %d, to "hip_wide"' % (
                "fit" if key == "gm_fit_backend" else "k-means", FORMS.EM_WIDE.lo, FORMS.EM_WIDE.hi, FORMS.EM_WIDE.step)
            raise ValueError('%s: "hip" fits mixtures on at most %d dimensions, prior "GMM" with code_size = %d needs the host fit '
                             '(leave %s out or set it to "sklearn"%s)' % (key, FORMS.EM_NARROW.hi, int(config["code_size"]), key, hint))


def _gather_ragged(parts, x, comm):
    for r, p_ in enumerate(parts):                                               # ranks with different sample counts: one broadcast each
        if r == comm.rank:
            p_.copy_(x)
        comm.broadcast_(p_, r)


def gather_samples(Xd, comm):
    """-> (every rank's samples in rank order, the offset of this rank's slice)."""
    if not comm.on:
        return Xd, 0
    Nl, R = Xd.shape
    counts = torch.zeros(comm.world, dtype=torch.int64, device=Xd.device)
    counts[comm.rank] = Nl
    comm.allreduce_(counts)
    cl = [int(c) for c in counts.cpu()]
    parts = [torch.empty(c, R, device=Xd.device) for c in cl]
    comm.dist.all_gather(parts, Xd, group=comm.group) if len(set(cl)) == 1 else _gather_ragged(parts, Xd, comm)
    return torch.cat(parts, 0), sum(cl[:comm.rank])


def initial_labels_for(backend, Xd, comm, K, rs, label_broadcast=None):
    """The hard labels of THIS rank's samples for a cold start: k-means needs every sample -- gathered once (rank order), labelled on
    rank 0, this rank keeps its slice.  `label_broadcast`: the hook of replicated fits inside a data-parallel job (rank 0's labels).
    `backend` = kmeans_backend: "hip" and "hip_wide" label the gathered DEVICE tensor (device_kmeans_labels, no copy to the host; DeviceKMeans picks
    the kernel family by the width), "sklearn" a host copy."""
    allx, off = gather_samples(Xd, comm)
    lab = torch.empty(allx.shape[0], dtype=torch.int32, device=Xd.device)
    if comm.rank == 0 and backend in DEVICE_KMEANS_BACKENDS:
        lab.copy_(device_kmeans_labels(allx, K, rs))
    elif comm.rank == 0:
        lab.copy_(torch.as_tensor(kmeans_labels(allx.cpu().numpy().astype(np.float64), K, rs)))
    comm.broadcast_(lab, 0)
    if label_broadcast is not None and not comm.on:
        label_broadcast(lab)
    return lab[off:off + Xd.shape[0]].contiguous()


def fit_plan(gm):
    """-> (cold start?, the random state of its k-means, fits to run): a fit starts from k-means labels, `n_init` times over, unless
    `warm_start` is set and an earlier fit left its state behind."""
    from sklearn.utils import check_random_state
    cold = not (gm.warm_start and gm._state is not None and hasattr(gm, "converged_"))
    return cold, check_random_state(gm.random_state), gm.n_init if cold else 1


def feed_tensors(K, R, device):
    """The fp32 copies (weights [K], means [K,R], covariances [K,R,R]) that a fit writes for the engine's mixture feed."""
    return torch.empty(K, device=device), torch.empty(K, R, device=device), torch.empty(K, R, R, device=device)


def iterate_until_done(estep, mstep, exchange, stats, flag, first_it, max_iter, check_every, what):
    """Enqueues estep(it) / exchange(stats) / mstep(it) for it = first_it, first_it + 1, ... and reads the device-side `done` flag
    every `check_every` iterations; the kernels are no-ops once it is set, so the result does not depend on `check_every`."""
    from .. import _lib as L
    it, done = first_it, False
    while not done:
        for _i in range(check_every):
            rc = estep(it)
            if exchange is not None:
                exchange(stats)
            rc = rc or mstep(it)
            if rc != 0:
                raise L.LadderHipError("%s failed: %s (%d)" % (what, L.ERRORS.get(rc, "?"), rc))
            it += 1
            if it > max_iter:
                break
        done = bool(flag.item() != 0) or it > max_iter                         # (identical on every rank: same all-reduced statistics)


# One family as fit_sliced drives it.  form: its row of mixture_forms.FAMILIES; moments(Xd, comm, f64, st, check) -> the all-reduced moments, having called
# check(global sample count) where sklearn checks it; e_mid(mom): the E-step's arguments between `state` and `stats`; m_mid: the M-step's between `state` and reg_covar
Family = collections.namedtuple("Family", "form moments e_mid m_mid what")


def fit_sliced(gm, X_local, comm, check_every, fam):
    """The fit of `gm` on THIS rank's samples `X_local` [N_local, R] with the kernels of `fam`: moments, then per restart and iteration
    E-step + local statistics / all-reduce of `stats` / M-step + convergence test, identical on every rank, against the device-side `done`
    flag (iterate_until_done).  A cold start takes its k-means labels from rank 0, once per restart; warm starts exchange statistics only.
    -> what best_of_restarts returns."""
    from .. import _lib as L
    K = gm.n_components
    Xd = device_samples(X_local, gm.device)
    Nl, R = Xd.shape
    st = torch.cuda.current_stream(gm.device).cuda_stream
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=gm.device)
    mom = fam.moments(Xd, comm, f64, st, lambda n: check_sample_count(n, K))    # sklearn's check, on the GLOBAL sample count
    form = fam.form
    stats = f64(L.query(form.stats_doubles, K, R))
    ws = torch.empty(L.query(form.workspace_bytes, Nl, K, R), dtype=torch.uint8, device=gm.device)
    do_init, rs, n_fits = fit_plan(gm)
    lib = L.load()
    estep_fn, mstep_fn = getattr(lib, form.estep), getattr(lib, form.mstep)
    n_state = L.query(form.state_doubles, K, R)

    def one_fit():
        state = f64(n_state) if do_init else gm._state
        state[FIT_CONVERGED:] = 0.0
        labels = gm._initial_labels(Xd, comm, rs) if do_init else None
        w, m, c = feed_tensors(K, R, gm.device)                    # (below: argument lists bound once, the loop is two foreign calls)
        e_head, e_tail = (Xd.data_ptr(), Nl, K, R), (state.data_ptr(),) + fam.e_mid(mom) + (stats.data_ptr(), ws.data_ptr(), ws.numel(), st)
        m_head = (stats.data_ptr(), mom.data_ptr(), K, R, state.data_ptr()) + fam.m_mid + (float(gm.reg_covar), float(gm.tol), gm.max_iter)
        m_tail = (w.data_ptr(), m.data_ptr(), c.data_ptr(), st)
        iterate_until_done(lambda it: estep_fn(*e_head, labels.data_ptr() if (labels is not None and it == 0) else None, *e_tail),
                           lambda it: mstep_fn(*m_head, it, *m_tail), comm.allreduce_ if comm.on else None, stats, state[FIT_DONE:],
                           0 if do_init else 1, gm.max_iter, check_every, fam.what)
        return state, w, m, c

    return best_of_restarts(n_fits, one_fit)


def read_tail(state):
    """(lower_bound_, n_iter_, converged_) of a finished fit -- one host synchronisation; raises sklearn's error on status -1."""
    tail = state[FIT_LB:].cpu().numpy()
    if tail[FIT_CONVERGED] < 0:
        raise ValueError(ILL_DEFINED)
    return float(tail[FIT_LB]), int(tail[FIT_NITER]), bool(tail[FIT_CONVERGED] > 0)


def best_of_restarts(n_restarts, run_one):
    """run_one() -> (state, *payload) of one finished fit; keeps the restart with the largest lower bound.
    -> (lower_bound_, n_iter_, converged_, state, *payload)."""
    best = None
    for _ in range(n_restarts):
        res = run_one()
        tail = read_tail(res[0])
        if best is None or tail[0] > best[0]:
            best = tail + tuple(res)
    return best


def keep_best(gm, best):
    """Stores what best_of_restarts returns on the mixture object `gm`, with sklearn's warning if that fit did not converge; -> gm."""
    gm.lower_bound_, gm.n_iter_, gm.converged_, gm._state, gm.weights_dev, gm.means_dev, gm.covariances_dev = best
    if not gm.converged_ and gm.max_iter > 0:
        from sklearn.exceptions import ConvergenceWarning
        warnings.warn(NOT_CONVERGED, ConvergenceWarning)
    return gm
