"""Contributed layers on top of the hot path (mirrors the reference's `ratinabox.contribs`): one module per class, imported
the reference's way —

    from ratinabox_amd.contribs.TaskEnvironment import TaskEnvironment
    from ratinabox_amd.contribs.ValueNeuron import ValueNeuron
    from ratinabox_amd.contribs.SuccessorFeatures import SuccessorFeatures
    from ratinabox_amd.contribs.PhasePrecessingPlaceCells import PhasePrecessingPlaceCells
    from ratinabox_amd.contribs.SubAgent import SubAgent, ThetaSequenceAgent, DumbAgent, ReplayAgent, ShiftAgent, UnrelatedAgent
    from ratinabox_amd.contribs.PlaneWaveNeurons import PlaneWaveNeurons
    from ratinabox_amd.contribs.NeuralNetworkNeurons import NeuralNetworkNeurons, MultiLayerPerceptron
"""
__all__ = ["TaskEnvironment", "ValueNeuron", "SuccessorFeatures", "PhasePrecessingPlaceCells", "SubAgent", "PlaneWaveNeurons",
           "NeuralNetworkNeurons"]
