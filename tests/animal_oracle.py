"""Float64 oracle of Stage-II for the SMAL animal types (chmosh.py:572-579, 613-617, 640-643): the human oracle's pieces
(oracle/stageii_oracle.py: forward, Jacobian, marker frames, max-mixture prior, rigid init, dogleg) with only what the animals add
restated here -- their free-variable sets, the horse's pose prior in the reference's own form (x - mean) . pic, the horse's
joint-angle term, and the frame loop that carries them.

animal_horse: poseB = (pose[3:84] - mean_pose[:81]) . pic[:81, :81] * wt_pose; poseB_jangles = exp(pose[p])^2 * wt_pose * 2 for the
12 ids p of smal_horse_joint_angle_prior (+3: the reference indexes pose[pose_body_ids]); both with wt_pose_first in the first-frame
rounds.  animal_dog: poseB = MaxMixtureComplete over the 93 ids of MaxMixtureDog * wt_pose, no joint-angle term."""
import numpy as np

from oracle import stageii_oracle as so

JANGLE_IDS = (6, 7, 8, 11, 12, 13, 20, 21, 22, 25, 26, 27)
DOG_JOINTS = (1, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 30, 31, 32, 33, 34)


def animal_pose_id_sets(model_type, NP, optimize_toes=False):
    """chmosh.py:546-579, 645-647, 665-667: (root, body, step1, step2)."""
    allp = list(range(NP))
    root = allp[:3]
    if model_type == 'animal_horse':
        body = allp[3:84]
    elif model_type == 'animal_dog':
        body = [allp[i] for i in np.arange(0, 105).reshape(-1, 3)[list(DOG_JOINTS)].reshape(-1)]
    else:
        raise ValueError(model_type)
    step1 = root + body
    if not optimize_toes:
        step1 = sorted(set(step1).difference(set(allp[30:36])))
    return root, body, list(step1), sorted(set(step1))


def horse_prior_raw(pkl, n=81):
    """smal_horse_prior(disable_tail_mouth_ear=True): (means[:81], pic[:81, :81])."""
    return dict(mean=np.asarray(pkl['mean_pose'], dtype=np.float64)[:n], pic=np.asarray(pkl['pic'], dtype=np.float64)[:n, :n])


def dog_prior_prepared(pkl):
    """MaxMixtureDog.get_gmm_prior restated (without its inverted determinant assert): the prepared mixture over the 93 ids."""
    ids = np.arange(0, 105).reshape(-1, 3)[list(DOG_JOINTS)].reshape(-1)
    covars = np.asarray(pkl['gmm_covs'], dtype=np.float64)[:, :, ids][:, ids]
    means = np.asarray(pkl['gmm_means'], dtype=np.float64)[:, ids]
    weights = np.asarray(pkl['gmm_weights'], dtype=np.float64).ravel()
    chols = np.asarray([np.linalg.cholesky(np.linalg.inv(c)) for c in covars])
    sqrdets = np.array([np.sqrt(np.linalg.det(c)) for c in covars])
    weights = weights / ((2 * np.pi) ** (len(ids) / 2.) * (sqrdets / sqrdets.min()))
    return {'means': means, 'chols': chols, 'weights': weights, 'npose': len(ids)}


class AnimalObjective(so.StageIIObjective):
    """StageIIObjective with the animal prior forms: `prior` is horse_prior_raw(...) (kind 'horse') or a prepared mixture ('dog')."""

    def __init__(self, m, closest, coef, prior, body_ids, kind):
        super().__init__(m, closest, coef, prior, body_ids)
        self.kind = kind
        self.jangle = np.asarray(JANGLE_IDS if kind == 'horse' else [], dtype=np.int64)

    def terms(self, pose, trans, shp=None):
        sim = self.markers_sim(pose, trans)
        out = {'data': ((sim[self.vis] - self.obs[self.vis]) * self.wt_data).ravel()}
        x = pose[self.body_ids]
        if self.kind == 'horse':
            out['poseB'] = (x - self.prior['mean']).dot(self.prior['pic']) * self.wt_pose
            out['poseB_jangles'] = np.exp(pose[self.jangle]) ** 2 * self.wt_pose * 2.
        else:
            out['poseB'] = so.gmm_prior_eval(self.prior, x)[0] * self.wt_pose
        if self.velo_target is not None:
            out['velo'] = (pose - self.velo_target) * self.wt_velo
        return out

    def J(self, x):
        pose, trans = self._unpack(x)
        body, kind, prior = self.body_ids, self.kind, self.prior
        # the data and velocity blocks as the human objective builds them (no prior, no finger / face / shape terms)
        self.body_ids = np.zeros(0, dtype=np.int64)
        try:
            Jd = so.StageIIObjective.J(self, x)
        finally:
            self.body_ids = body
        n = Jd.shape[1]
        nobs3 = 3 * int(self.vis.sum())
        pos = {int(pid): i for i, pid in enumerate(self.free_ids)}
        if kind == 'horse':
            Jp = prior['pic'].T                                      # d ((x - mu) . P) / dx
        else:
            _, _, Jp = so.gmm_prior_eval(prior, pose[body], want_jac=True)
        Jb = np.zeros((Jp.shape[0], n))
        for bi, pid in enumerate(body):
            if int(pid) in pos:
                Jb[:, 3 + pos[int(pid)]] = Jp[:, bi]
        blocks = [Jd[:nobs3], Jb * self.wt_pose]
        if kind == 'horse':
            Jj = np.zeros((len(self.jangle), n))
            r = np.exp(pose[self.jangle]) ** 2 * self.wt_pose * 2.
            for i, pid in enumerate(self.jangle):
                if int(pid) in pos:
                    Jj[i, 3 + pos[int(pid)]] = 2.0 * r[i]
            blocks.append(Jj)
        blocks.append(Jd[nobs3:])                                   # velocity rows (if any)
        return np.vstack(blocks)


class AnimalObjectiveFD(AnimalObjective):
    """The same residuals with the Jacobian the executed-reference fixture was made with: central differences, h = 1e-6
    (tests/golden/make_ref_stageii_golden.py: minimize) -- the like-for-like comparison with that fixture."""

    def J(self, x):
        h = 1e-6
        cols = []
        for i in range(len(x)):
            xp = x.copy(); xp[i] += h
            xm = x.copy(); xm[i] -= h
            cols.append((self.r(xp) - self.r(xm)) / (2 * h))
        return np.array(cols).T


def animal_chain(m, prior, closest, coef, obs, vis, model_type, weights=None, optimize_toes=False, maxiter=100,
                 num_train_markers=46, init=None, fd_jacobian=False):
    """The frame loop of chmosh.py:584-724 for an animal model; same return layout as stageii_chain (errs keyed as the reference's
    stageii_errs: data, poseB, poseB_jangles (horse), velo).  fd_jacobian: AnimalObjectiveFD instead of the analytic Jacobian."""
    W = so.stageii_weights_default() if weights is None else dict(weights)
    kind = 'horse' if model_type == 'animal_horse' else 'dog'
    root, body, step1, step2 = animal_pose_id_sets(model_type, m['NP'], optimize_toes)
    objf = (AnimalObjectiveFD if fd_jacobian else AnimalObjective)(m, closest, coef, prior, body, kind)
    M, F = closest.shape[0], obs.shape[0]
    pose_prev, first = None, True
    if init is not None:
        objf.pose = np.array(init['pose'], dtype=np.float64)
        objf.trans = np.array(init['trans'], dtype=np.float64)
        pose_prev = None if init.get('pose_prev') is None else np.array(init['pose_prev'], dtype=np.float64)
        first = False
    out = dict(fullpose=[], trans=[], frame_ids=[], pose=[], errs={}, iters=[], markers_sim=[])
    for t in range(F):
        vmask = np.asarray(vis[t], dtype=bool)
        n_obs = int(vmask.sum())
        if n_obs == 0:
            continue
        anneal = 1.0 + ((M - n_obs) / M) * W['stageii_wt_annealing'] if n_obs < M else 1.0
        objf.vis, objf.obs = vmask, np.asarray(obs[t], dtype=np.float64)
        objf.wt_data = W['stageii_wt_data'] * (num_train_markers / n_obs)
        wt_pose = W['stageii_wt_poseB'] * anneal
        objf.wt_velo = W['stageii_wt_velo']
        objf.velo_target = None if pose_prev is None else objf.pose + (objf.pose - pose_prev)
        st = {}
        if first:
            sim = objf.markers_sim()
            R, T = so.rigid_landmark_transform(sim[vmask].T, objf.obs[vmask].T)
            objf.pose[:3] = so.rotmat_to_rotvec(R)
            objf.trans[:] = T.ravel()
            for s in (10., 5., 1.):
                objf.wt_pose = s * wt_pose
                objf.free_ids = step1
                objf.set_x(so.minimize_dogleg(objf, objf.x(), e_3=1e-3, delta_0=.5, maxiter=maxiter, stats=st))
            first = False
        else:
            pose_prev = objf.pose.copy()
        objf.wt_pose = wt_pose
        for ids in (step1, step2):
            objf.free_ids = ids
            objf.set_x(so.minimize_dogleg(objf, objf.x(), e_3=1e-2, delta_0=.5, maxiter=maxiter, stats=st))
        for k, v in objf.terms(objf.pose, objf.trans).items():
            out['errs'].setdefault(k, []).append(float(np.sum(v ** 2)))
        out['markers_sim'].append(objf.markers_sim()[vmask].copy())
        out['fullpose'].append(so.fullpose_from_pose(m, objf.pose))
        out['trans'].append(objf.trans.copy())
        out['pose'].append(objf.pose.copy())
        out['frame_ids'].append(t)
        out['iters'].append(st.get('iterations', 0))
    return dict(fullpose=np.array(out['fullpose']), trans=np.array(out['trans']), pose=np.array(out['pose']),
                frame_ids=np.array(out['frame_ids'], dtype=np.int64), errs={k: np.array(v) for k, v in out['errs'].items()},
                iters=np.array(out['iters']), markers_sim=out['markers_sim'],
                final=dict(pose=objf.pose.copy(), trans=objf.trans.copy(), pose_prev=None if pose_prev is None else pose_prev.copy()))


# ---- seeded cases (synth.make_sequence of an animal type) for the oracle and for libmoshii ------------------------------------------
def animal_case(model_type='animal_horse', F=6, M=40, seed=1, **kw):
    from moshpp_amd import synth
    s = synth.make_sequence(model_type, F, M, seed=seed, body_only_markers=False, **kw)
    dd = s['model']
    K = synth.MODEL_DIMS[model_type][1]
    model = dict(v_template=dd['v_template'], shapedirs=dd['shapedirs'], posedirs=dd['posedirs'], weights=dd['weights'],
                 J_regressor=dd['J_regressor'], parents=synth.kintree_parents(model_type), body_dof=3 * K, hand_dof=0,
                 hands_mean=None, selected_components=None)
    m = so.prepare_model(model, s['betas'])
    can = so.verts_forward(m, so.fullpose_from_pose(m, np.zeros(m['NP'])), np.zeros(3))
    closest, coef = so.transformed_coeffs(can, s['markers_latent'])
    pkl = s['animal_prior']
    prior = horse_prior_raw(pkl) if model_type == 'animal_horse' else dog_prior_prepared(pkl)
    return dict(s=s, m=m, model=model, can=can, closest=closest, coef=coef, prior=prior, pkl=pkl,
                obs=np.nan_to_num(s['markers']), vis=~np.isnan(s['markers']).any(-1), model_type=model_type)


def animal_device_case(case, optimize_toes=False, maxiter=100):
    """libmoshii handles + options of an animal_case, through the product's own host setup (prior.py, chmosh.stageii_pose_ids)."""
    from moshpp_amd import capi, chmosh, prior as mprior
    mdl = case['model']
    dev = capi.Model(mdl['v_template'], mdl['shapedirs'], mdl['posedirs'], mdl['weights'], mdl['J_regressor'], mdl['parents'],
                     mdl['body_dof'], 0, None, None)
    dev.set_betas(case['s']['betas'])
    att = capi.Attachment(dev, case['closest'], case['coef'])
    p = mprior.create_body_prior(case['model_type'], case['pkl'])
    pr = capi.Prior(p['means'], p['chols'], p['weights'])
    ids = chmosh.stageii_pose_ids(case['model_type'], case['m']['NP'], False, optimize_toes)
    horse = case['model_type'] == 'animal_horse'
    opts = capi.make_opts(so.stageii_weights_default(), ids['step1'], ids['step2'], ids['body'], [], maxiter=maxiter,
                          jangle_ids=chmosh.STAGEII_JANGLE_IDS if horse else ())
    return dict(model=dev, attach=att, prior=pr, opts=opts)


def animal_ref_case(model_type, F, M, seed, n_verts, empty_frames=(), dropout=0.02, outdir=None):
    """The seeded inputs of tests/golden/make_ref_stageii_animal_golden.py: a triangulated synthetic quadruped of `n_verts` vertices
    (small enough for the generator's finite-difference Jacobian of the reference's residuals), its prior pickle and the sequence;
    with `outdir` the model / prior / mocap files are written as the reference reads them.  Returns an animal_case-like dict."""
    import pickle
    from moshpp_amd import synth
    dd = synth.synth_mesh_model(model_type, seed=seed, n_verts=n_verts)
    s = synth.make_sequence(model_type, F, M, seed=seed, dd=dd, body_only_markers=False, n_gaps=1, dropout=dropout,
                            empty_frames=tuple(empty_frames))
    K = synth.MODEL_DIMS[model_type][1]
    model = dict(v_template=dd['v_template'], shapedirs=dd['shapedirs'], posedirs=dd['posedirs'], weights=dd['weights'],
                 J_regressor=dd['J_regressor'], parents=synth.kintree_parents(model_type), body_dof=3 * K, hand_dof=0,
                 hands_mean=None, selected_components=None)
    m = so.prepare_model(model, s['betas'])
    can = so.verts_forward(m, so.fullpose_from_pose(m, np.zeros(m['NP'])), np.zeros(3))
    closest, coef = so.transformed_coeffs(can, s['markers_latent'])
    pkl = s['animal_prior']
    out = dict(s=s, m=m, model=model, can=can, closest=closest, coef=coef, pkl=pkl, model_type=model_type,
               prior=horse_prior_raw(pkl) if model_type == 'animal_horse' else dog_prior_prepared(pkl),
               obs=np.nan_to_num(s['markers']), vis=~np.isnan(s['markers']).any(-1))
    if outdir is not None:
        import os
        out['model_fname'] = os.path.join(outdir, 'model.pkl')
        with open(out['model_fname'], 'wb') as fh:
            import scipy.sparse as sp
            pk = {k: v for k, v in dd.items() if not k.startswith('_') and k != 'model_type'}
            pk['J_regressor'] = sp.csc_matrix(dd['J_regressor'])     # (as the model pickles ship it)
            pickle.dump(pk, fh, protocol=2)
        out['prior_fname'] = os.path.join(outdir, 'prior.pkl')
        with open(out['prior_fname'], 'wb') as fh:
            pickle.dump(pkl, fh, protocol=2)
        out['mocap_fname'] = os.path.join(outdir, 'mocap.npz')
        np.savez(out['mocap_fname'], markers=s['markers'], labels=np.array(s['labels']), frame_rate=s['frame_rate'])
    return out
