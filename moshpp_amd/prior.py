"""Max-mixture GMM body-pose prior, host-side preparation.

Mirror of `create_gmm_body_prior` (reference src/moshpp/prior/gmm_prior_ch.py:107-134) and of the two SMAL animal priors
(prior/horse_body_prior.py `smal_horse_prior`, prior/dog_body_prior.py `MaxMixtureDog`).  Evaluation (`MaxMixtureComplete`,
:42-85) runs inside the HIP chain kernel; this module only prepares the constants, every prior in the one form the kernel takes:
dict(means[G,npose], chols[G,npose,npose] lower, weights[G], npose).
"""
from __future__ import annotations

import os
import pickle

import numpy as np


def _load_mixture(source):
    if isinstance(source, dict):
        return source
    if not os.path.exists(source):
        raise AssertionError(ValueError(f'pose_body_prior_fname does not exist: {source}'))
    with open(source, 'rb') as fh:
        return pickle.load(fh, encoding='latin-1')


def create_gmm_body_prior(pose_body_prior_fname, exclude_hands=False):
    """-> dict(means[G,npose], chols[G,npose,npose], weights[G], npose).
    `pose_body_prior_fname` is the pickle path (keys 'means', 'covars', 'weights') or such a dict.

    Per component g the kernel needs a factor L_g with L_g L_g^T = Sigma_g^-1 (the residual is L_g^T (x - mu_g)) and the mixture
    weight divided by the Gaussian's normalisation, (2 pi)^(npose/2) sqrt(det Sigma_g), the determinants taken relative to the
    smallest one (gmm_prior_ch.py:121-131).  Both come out of ONE Cholesky factorisation of the covariance block here,
    Sigma_g = C C^T:  det Sigma_g = prod(diag C)^2, Sigma_g^-1 = C^-T C^-1 -- whose lower Cholesky factor (unique: positive diagonal)
    is obtained by factorising the explicitly symmetrised inverse."""
    mix = _load_mixture(pose_body_prior_fname)
    npose = 63 if exclude_hands else 69
    mu = np.ascontiguousarray(np.asarray(mix['means'], dtype=np.float64)[:, :npose])
    sigma = np.asarray(mix['covars'], dtype=np.float64)[:, :npose, :npose]
    pi_g = np.asarray(mix['weights'], dtype=np.float64).ravel()
    factors = np.empty_like(sigma)
    root_det = np.empty(len(sigma))
    for g, cov in enumerate(sigma):
        root_det[g] = np.sqrt(np.linalg.det(cov))
        factors[g] = np.linalg.cholesky(np.linalg.inv(cov))
    norm = (2.0 * np.pi) ** (0.5 * npose) * (root_det / root_det.min())
    return dict(means=mu, chols=np.ascontiguousarray(factors), weights=pi_g / norm, npose=npose)


# SMAL dog: the joints whose pose entries the prior covers (dog_body_prior.py MaxMixtureDog.get_gmm_prior, chmosh.py:574-579)
DOG_PRIOR_JOINTS = (1, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 30, 31, 32, 33, 34)


def dog_pose_body_ids():
    """The 93 pose ids of DOG_PRIOR_JOINTS (not contiguous)."""
    return [3 * j + c for j in DOG_PRIOR_JOINTS for c in range(3)]


def smal_horse_prior(pose_body_prior_fname, disable_tail_mouth_ear=True):
    """smal_horse_prior (horse_body_prior.py): the residual (x - mean_pose[:n]) . pic[:n, :n], n = 81 (105 without
    `disable_tail_mouth_ear`; chmosh.py only ever uses 81), as the one-component max-mixture the kernel evaluates.
    The pickle holds 'pic' [105, 105] and 'mean_pose' [105].

    The kernel's residual of a component is sqrt(1/2) L^T (x - mu) with L lower triangular, plus -log w; |(x - mu) . P|^2 =
    (x - mu)^T P P^T (x - mu), so L = chol(2 P P^T) and w = 1 give the reference's value, gradient and J^T J to round-off
    (the residual vectors differ by an orthogonal map; `P` itself is not triangular and cannot be passed as it is)."""
    res = _load_mixture(pose_body_prior_fname)
    n = 81 if disable_tail_mouth_ear else np.asarray(res['mean_pose']).size
    P = np.asarray(res['pic'], dtype=np.float64)[:n, :n]
    mu = np.asarray(res['mean_pose'], dtype=np.float64).ravel()[:n]
    A = 2.0 * P.dot(P.T)
    L = np.linalg.cholesky(0.5 * (A + A.T))
    return dict(means=np.ascontiguousarray(mu[None]), chols=np.ascontiguousarray(L[None]), weights=np.ones(1), npose=n)


def create_dog_gmm_prior(pose_body_prior_fname):
    """MaxMixtureDog.get_gmm_prior (dog_body_prior.py): the mixture 'gmm_means' [G, 105], 'gmm_covs' [G, 105, 105],
    'gmm_weights' [G] restricted to the 93 pose entries of DOG_PRIOR_JOINTS; factors chol(inv(cov)), weights normalised as
    the human prior's.  The reference's `assert np.any(sqrdets == 0.0)` is inverted (it fails for every positive-definite
    covariance unless Python runs with -O); the intent -- refuse a singular covariance -- is what is checked here."""
    gmm = _load_mixture(pose_body_prior_fname)
    ids = np.asarray(dog_pose_body_ids())
    covars = np.asarray(gmm['gmm_covs'], dtype=np.float64)[:, :, ids][:, ids]
    means = np.ascontiguousarray(np.asarray(gmm['gmm_means'], dtype=np.float64)[:, ids])
    weights = np.asarray(gmm['gmm_weights'], dtype=np.float64).ravel()
    npose = len(ids)
    sqrdets = np.array([np.sqrt(np.linalg.det(c)) for c in covars])
    if np.any(sqrdets == 0.0):      # (before the factorisation, which a singular covariance would stop first)
        raise ValueError(f'Encountered zeros in the determinant of the covariance matrix: {sqrdets}')
    chols = np.ascontiguousarray([np.linalg.cholesky(np.linalg.inv(cov)) for cov in covars])
    const = (2 * np.pi) ** (npose / 2.)
    return dict(means=means, chols=chols, weights=weights / (const * (sqrdets / sqrdets.min())), npose=npose)


def create_body_prior(model_type, pose_body_prior_fname):
    """The pose prior `mosh_stageii` builds for a model type (bodymodel_loader.py:121-135); None for MANO."""
    if model_type == 'mano':
        return None
    if model_type == 'animal_horse':
        return smal_horse_prior(pose_body_prior_fname)
    if model_type == 'animal_dog':
        return create_dog_gmm_prior(pose_body_prior_fname)
    return create_gmm_body_prior(pose_body_prior_fname, exclude_hands=model_type in ['smplh', 'smplx'])
