"""Losses that stay on the device until somebody looks: the update leaves the operands of the loss in buffers that stay valid
until the next update of the same kind writes them, and no reduction launch sits inside the iteration."""


class LazyLoss(object):
    """``expr(*operands)``, evaluated by ``float(x)`` / ``x.detach()`` only."""

    def __init__(self, expr, *operands):
        self.expr, self.operands = expr, operands

    def detach(self):
        return self.expr(*self.operands)

    def __float__(self):
        return float(self.detach())


class LazySum(LazyLoss):
    """Per-workgroup loss partials (``parts``), summed only when somebody looks."""

    def __init__(self, parts):
        LazyLoss.__init__(self, lambda p: p.sum(), parts)
        self.parts = parts
