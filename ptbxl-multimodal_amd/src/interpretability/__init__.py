"""Interpretability tools: `grad_cam_1d.GradCAM1D`, the reference's Grad-CAM class on top of `ecg_hip.gradcam`."""
