"""Golden vectors for categorical action spaces of more than 64 classes: the reference's ``Categorical``
(``src/rl8/distributions.py:125-132``) and ``ppo_losses`` (``src/rl8/nn/functional.py:259-363``) at 65, 100 and 1000
classes, and its ``Algorithm`` on the tests' walk environment with 100 actions through ``collect()`` / ``step()``.

Like the other generators beside it this runs only where the reference is checked out next to the repository; it
imports the reference unmodified through ``generate_fixtures`` (which supplies ``record_ppo_case``,
``draw_exponential_like``, ``walk_env``, ``gen_env_first_update`` and ``save_reproducible``) only when it generates.
The fixtures hold arrays only.

``wide_categorical.npz``
    ``ppo_*`` cases: inputs, the five losses and the autograd gradients, as ``ppo_losses.npz`` holds them;
    ``cat*`` cases: logits, torch's own multinomial noise, the classes it picked, their log-probabilities and the modes,
    as ``samplers.npz`` holds them.  m = 8 rows; k in {65, 100, 1000}; a in {1, 2}.  No recorded draw has its two
    largest ratios p / q closer than 1e-4 relative (asserted here), so the picks are held bit for bit.

``first_update_ff_walk100.npz`` and its ``_init`` / ``_grad`` / ``_final`` companions
    ``gen_env_first_update`` on ``walk_env(4, 100)``: what ``first_update_ff_walk4.npz`` holds for four actions.  The
    three copies of the model's weights (initial, first clipped gradient, after one update) go to files of their own so
    that every file stays under 1 MiB; the main file keeps everything else under the names ``gen_env_first_update``
    gives them.  The smallest top-two gap over the recorded draws is stored as ``min_top_two_gap``.

Usage::

    python tests/golden/generate_wide_categorical_fixtures.py

"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

M = 8
CLASSES = (65, 100, 1000)
DIMS = (1, 2)
GAP = 1e-4
MIB = 1 << 20

HPS = {
    "p0": dict(clip_param=0.2, dual_clip_param=None, entropy_coeff=0.0, vf_clip_param=5.0, vf_coeff=1.0),
    "p1": dict(clip_param=0.2, dual_clip_param=5.0, entropy_coeff=0.0, vf_clip_param=5.0, vf_coeff=1.0),
    "p2": dict(clip_param=0.3, dual_clip_param=None, entropy_coeff=1e-2, vf_clip_param=1.0, vf_coeff=0.5),
    "p3": dict(clip_param=0.1, dual_clip_param=3.0, entropy_coeff=1e-2, vf_clip_param=2.0, vf_coeff=2.0),
}
#: one set of hyperparameters per (k, a): plain, dual clip, entropy, both -- each of the last two also at 1000 classes
HP_OF = {(65, 1): "p0", (65, 2): "p1", (100, 1): "p2", (100, 2): "p3", (1000, 1): "p3", (1000, 2): "p2"}


def top_two_gap(probs: torch.Tensor, q: torch.Tensor) -> float:
    top = (probs.double() / q.double()).topk(2, dim=-1).values
    return float(((top[..., 0] - top[..., 1]) / top[..., 0]).min())


def gen_wide_categorical(gf) -> None:
    from rl8.distributions import Categorical
    from tensordict import TensorDict

    arrays: dict = {}
    cases: list = []
    g = torch.Generator().manual_seed(65)
    for ncls in CLASSES:
        for adim in DIMS:
            hname = HP_OF[ncls, adim]
            adv = torch.randn(M, 1, generator=g)
            returns = torch.randn(M, 1, generator=g) * 3
            values = (returns + torch.randn(M, 1, generator=g) * 2).requires_grad_(True)
            logits = (torch.randn(M, adim, ncls, generator=g) * 1.5).requires_grad_(True)
            actions = torch.randint(0, ncls, (M, adim), generator=g)
            dist = Categorical(TensorDict({"logits": logits}, batch_size=[M]), None)
            with torch.no_grad():
                logp_old = dist.logp(actions) + torch.randn(M, 1, generator=g) * 0.4
            gf.record_ppo_case(arrays, cases, f"ppo_k{ncls}_a{adim}_{hname}", dist, actions, logp_old, adv, returns,
                               values, {"logits": logits}, HPS[hname])
    arrays["cases"] = np.array(cases)

    torch.manual_seed(100)
    sampler_cases = []
    for ncls in CLASSES:
        for adim in DIMS:
            name = f"cat_k{ncls}_a{adim}"
            logits = torch.randn(M, adim, ncls) * 2.0
            dist = Categorical(TensorDict({"logits": logits}, batch_size=[M]), None)
            probs = dist.dist.probs.reshape(-1, ncls)
            q = gf.draw_exponential_like(probs)
            actions = dist.sample()
            check = torch.argmax(probs / q, dim=-1).reshape(M, adim)
            assert (check == actions).all(), "multinomial != argmax(p/q): torch changed"
            assert top_two_gap(probs, q) > GAP, (name, top_two_gap(probs, q))
            arrays[f"{name}_logits"] = logits
            arrays[f"{name}_q"] = q.reshape(M, adim, ncls)
            arrays[f"{name}_actions"] = actions
            arrays[f"{name}_logp"] = dist.logp(actions)
            arrays[f"{name}_mode"] = dist.deterministic_sample()
            sampler_cases.append(name)
    arrays["sampler_cases"] = np.array(sampler_cases)
    gf.save_reproducible("wide_categorical.npz", **arrays)
    assert os.path.getsize(os.path.join(HERE, "wide_categorical.npz")) < MIB // 2


def gen_walk100_first_update(gf) -> None:
    """``gf.gen_env_first_update`` as it is; its one ``save`` call is caught and the arrays are split over four files.
    ``torch.distributions.Categorical.sample`` is wrapped underneath ``gf.Recorder`` (which wraps it again and records
    the noise) to measure the top-two gap of every draw of both runs."""
    gaps: list = []
    real_sample = torch.distributions.Categorical.sample

    def sample(dist, sample_shape=torch.Size()):
        probs = dist.probs.reshape(-1, dist._num_events)
        gaps.append(top_two_gap(probs, gf.draw_exponential_like(probs)))
        return real_sample(dist, sample_shape)

    caught: dict = {}
    real_save = gf.save

    def save(name, **arrays):
        assert name == "first_update_ff_walk100.npz"
        caught.update(arrays)

    torch.distributions.Categorical.sample = sample
    gf.save = save
    try:
        gf.gen_env_first_update("first_update_ff_walk100.npz", gf.walk_env(4, 100))
    finally:
        torch.distributions.Categorical.sample = real_sample
        gf.save = real_save
    assert len(gaps) >= 2 * 32 and caught["it0_cat_q"].shape == (32, 64, 1, 100)
    assert min(gaps) > GAP, min(gaps)
    caught["min_top_two_gap"] = np.float64(min(gaps))
    parts = {"_init": "init_", "_grad": "sgd1_grad_", "_final": "sgd1_final_"}
    for suffix, prefix in parts.items():
        part = {k: v for k, v in caught.items() if k.startswith(prefix)}
        assert part
        gf.save_reproducible(f"first_update_ff_walk100{suffix}.npz", **part)
    main = {k: v for k, v in caught.items() if not k.startswith(tuple(parts.values()))}
    gf.save_reproducible("first_update_ff_walk100.npz", **main)
    for suffix in ("", *parts):
        assert os.path.getsize(os.path.join(HERE, f"first_update_ff_walk100{suffix}.npz")) < MIB, suffix


def main() -> None:
    sys.path.insert(0, HERE)
    import generate_fixtures as gf

    gen_wide_categorical(gf)
    gen_walk100_first_update(gf)


if __name__ == "__main__":
    main()
