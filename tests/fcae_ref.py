"""Plain-torch restatement of the reference's FullyConnectedAutoencoder (models/FullyConnected.py:65-104,
118-159) for the tests: CPU or GPU, any floating dtype (``.double()`` gives the fp64 yardstick).  It imports
neither the package under test nor the oracle.  tools/gen_fcae_golden.py asserts that in fp32 it reproduces
the reference's own class bit for bit (outputs and all 30 gradients, train and eval mode)."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class GradReverse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x

    @staticmethod
    def backward(ctx, g):
        return -g.clone()


class StatisticsPooling(nn.Module):
    """speechbrain.nnet.pooling.StatisticsPooling without lengths: (mean, unbiased std + 1e-5) over time.
    ``noise``: None -> no offset on the mean; a tensor [B, C] in [0, 1] -> eps * ((1 - 9) noise + 9) is added
    (speechbrain draws it from a rescaled gaussian on every call)."""

    def __init__(self):
        super().__init__()
        self.eps = 1e-5
        self.noise = None

    def forward(self, x):
        mean = x.mean(dim=1)
        std = x.std(dim=1)
        if self.noise is not None:
            mean = mean + self.eps * ((1 - 9) * self.noise.to(mean) + 9)
        std = std + self.eps
        return torch.cat((mean, std), dim=1).unsqueeze(1)


class FullyConnSexClassifier(nn.Module):
    def __init__(self, num_classes=2):
        super().__init__()
        self.initial = nn.Sequential(nn.Linear(20, 40), nn.ReLU(), nn.Linear(40, 40), nn.ReLU())
        self.norm = nn.BatchNorm1d(20)
        self.classify = nn.Sequential(
            nn.Linear(80, 40), nn.BatchNorm1d(40), nn.ReLU(), nn.Linear(40, 40), nn.ReLU(), nn.Linear(40, 20),
            nn.BatchNorm1d(20), nn.Linear(20, num_classes))
        self.stats_pooling = StatisticsPooling()

    def forward(self, x):
        x = GradReverse.apply(x)
        x = x.reshape(x.shape[0], x.shape[2], x.shape[1])         # a reinterpretation, not a transpose
        x = self.norm(x)
        x = x.reshape(x.shape[0], x.shape[2], x.shape[1])
        u = self.initial(x)
        pooled = self.stats_pooling(u).squeeze(1)
        return F.log_softmax(self.classify(pooled), 1)


class FullyConnectedAutoencoder(nn.Module):
    def __init__(self, mfcc_feature_dim=80, batch_size=None):
        super().__init__()
        self.mfcc_feature_dim, self.batch_size = mfcc_feature_dim, batch_size
        self.encoder = nn.Sequential(nn.Linear(mfcc_feature_dim, 60), nn.ReLU(), nn.Linear(60, 40), nn.ReLU(),
                                     nn.Linear(40, 20))
        self.decoder = nn.Sequential(nn.Linear(20, 40), nn.ReLU(), nn.Linear(40, 60), nn.ReLU(),
                                     nn.Linear(60, mfcc_feature_dim))
        self.sex_classifier = FullyConnSexClassifier(2)

    def forward(self, x):
        z = self.encoder(x)
        logp = self.sex_classifier(z)
        return self.decoder(z), logp


def loss_fn(recon, logp, target, gender, w_recon=0.5, w_sex=0.5):
    """w_recon * MSE + w_sex * NLL, the objective of the fcae tests"""
    B = recon.shape[0]
    return w_recon * F.mse_loss(recon.reshape(B, -1), target.reshape(B, -1)) + w_sex * F.nll_loss(logp, gender)


def relmse(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float(((a - b) ** 2).sum() / (b ** 2).sum().clamp_min(1e-300))


def run_step(model, feats, gender, train=True, w_recon=0.5, w_sex=0.5):
    """one forward (+ backward in train mode) -> dict(recon, logp, loss, grads, buffers)"""
    model.train(train)
    model.zero_grad(set_to_none=True)
    with torch.set_grad_enabled(train):
        recon, logp = model(feats)
        loss = loss_fn(recon, logp, feats, gender, w_recon, w_sex)
    grads = {}
    if train:
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    return dict(recon=recon.detach(), logp=logp.detach(), loss=loss.detach(), grads=grads,
                buffers={k: v.detach().clone() for k, v in model.named_buffers()})
